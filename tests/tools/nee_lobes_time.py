"""Light sampling at rough metal and medium vertices (HRT_FLAG_NEE_LOBES) against the same render without the flag: for
the fog room and the brushed floor of tests/test_gpu_nee_lobes.py (256x256, 64 spp, --nee) and shiny_teapot.yaml (640x640, 100 spp,
--nee-env, the bench's stand-in assets) prints the frame time (host wall clock around hrt_render_stripes, best of `--reps`), the path
segments, the shadow rays and the RMS error of the linear film against a high-spp reference (`--ref-mult` x spp, seed 1, the mean of
both estimators' films: independent of the films compared).  Then an equal-time row: the flag at the sample count whose measured time
matches the render's without it, and its RMS error.
  python3 tests/tools/nee_lobes_time.py [--reps 3] [--ref-mult 8]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from hobbyraytracer_amd import api  # noqa: E402
from tests.test_gpu_nee_lobes import BRUSHED_FLOOR_YAML, FOG_ROOM_YAML  # noqa: E402


def best(fn, reps):
    out, t = None, float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t = min(t, time.perf_counter() - t0)
    return out, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-mult", type=int, default=8)
    a = ap.parse_args()
    d = tempfile.mkdtemp()
    api.write_teapot_obj(os.path.join(d, "teapot.obj"), 1.0)
    api.write_hall_hdr(os.path.join(d, "old_hall_4k.hdr"), 4096, 2048)
    for name, yaml in (("fog_room", FOG_ROOM_YAML), ("brushed_floor", BRUSHED_FLOOR_YAML)):
        with open(os.path.join(d, name + ".yaml"), "w") as f:
            f.write(yaml)
    golden = os.path.join(ROOT, "tests", "golden", "scenes")
    for scene, path, W, H, spp, base in (("fog_room", os.path.join(d, "fog_room.yaml"), 256, 256, 64, dict(nee=True)),
                                         ("brushed_floor", os.path.join(d, "brushed_floor.yaml"), 256, 256, 64, dict(nee=True)),
                                         ("shiny_teapot", os.path.join(golden, "shiny_teapot.yaml"), 640, 640, 100, dict(nee_env=True))):
        hs = api.HostScene(path, d)
        dev = api.DeviceScene(hs.flat_ptr, 0)
        cam = hs.camera(W, H)
        ref = np.zeros((H, W, 3))
        for lobes in (False, True):
            img, _ = dev.render_stripes(cam, api.default_params(W, H, spp * a.ref_mult, seed=1, nee_lobes=lobes, **base), 8, 0, 1)
            ref += 0.5 * img.astype(np.float64)
        rms = lambda img: float(np.sqrt(np.mean((img.astype(np.float64) - ref) ** 2)))   # noqa: E731
        times = {}
        for lobes in (False, True):
            p = api.default_params(W, H, spp, nee_lobes=lobes, **base)
            dev.render_stripes(cam, p, 8, 0, 1)
            (img, st), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), a.reps)
            times[lobes] = t
            print(f"{scene} {W}x{H} {spp}spp  {sorted(base)[0]}{' + nee_lobes' if lobes else '            '}  {t * 1e3:7.1f} ms  rays {st.rays:>12d}"
                  f"  shadow_rays {st.shadow_rays:>12d}  rms {rms(img):.5g}", flush=True)
        # equal time: start from the ratio of the two times, then correct twice from what was measured
        n_eq, t = spp * times[False] / times[True], times[True]
        for _ in range(3):
            n_try = max(1, int(round(n_eq)))
            p = api.default_params(W, H, n_try, nee_lobes=True, **base)
            (img, _), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), a.reps)
            n_eq = n_try * times[False] / t
        print(f"{scene} {W}x{H} {n_try}spp  + nee_lobes (equal time)  {t * 1e3:7.1f} ms (without {times[False] * 1e3:.1f} ms)  rms {rms(img):.5g}", flush=True)
        dev.close()


if __name__ == "__main__":
    main()
