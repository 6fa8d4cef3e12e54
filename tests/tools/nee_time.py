"""Next-event estimation (HRT_FLAG_NEE) against the default estimator: for cornell_box.yaml (256x256, 256 spp) and the
headline frame (teapot_scene.yaml 640x640, 100 spp, the bench's stand-in assets) prints the frame time (host wall clock around
hrt_render_stripes, best of `--reps`; also the default render without the tail kernel, the schedule NEE runs on), the path segments, the shadow rays and the RMS error of the linear film against a high-spp
reference (`--ref-mult` x spp, seed 1, the mean of both estimators' films: independent of the films compared).  Then an equal-time row:
NEE at the sample count whose measured time matches the default render's, and its RMS error.
  python3 tests/tools/nee_time.py [--reps 3] [--ref-mult 8]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from hobbyraytracer_amd import api  # noqa: E402


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
    for scene, W, H, spp in (("cornell_box.yaml", 256, 256, 256), ("teapot_scene.yaml", 640, 640, 100)):
        hs = api.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", scene), d)
        dev = api.DeviceScene(hs.flat_ptr, 0)
        cam = hs.camera(W, H)
        ref = np.zeros((H, W, 3))
        for nee in (False, True):
            img, _ = dev.render_stripes(cam, api.default_params(W, H, spp * a.ref_mult, seed=1, nee=nee), 8, 0, 1)
            ref += 0.5 * img.astype(np.float64)
        rms = lambda img: float(np.sqrt(np.mean((img.astype(np.float64) - ref) ** 2)))   # noqa: E731
        times = {}
        for nee in (False, True):
            p = api.default_params(W, H, spp, nee=nee)   # (rays and shadow_rays are counted without HRT_FLAG_STATS)
            dev.render_stripes(cam, p, 8, 0, 1)
            (img, st), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), a.reps)
            times[nee] = t
            print(f"{scene} {W}x{H} {spp}spp  {'nee    ' if nee else 'default'}  {t * 1e3:7.1f} ms  rays {st.rays:>12d}"
                  f"  shadow_rays {st.shadow_rays:>12d}  rms {rms(img):.5g}", flush=True)
        # equal time: the sample count whose MEASURED NEE time matches the default render's (the fixed per-batch cost makes time
        # not proportional to spp: start from the ratio, then correct twice from what was measured)
        # what NEE's round-by-round schedule costs by itself: the default render without the tail kernel (HRT_WF_TAIL_ROUND >= max_depth)
        os.environ["HRT_WF_TAIL_ROUND"] = "1000000"
        p = api.default_params(W, H, spp)
        dev.render_stripes(cam, p, 8, 0, 1)
        _, t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), a.reps)
        del os.environ["HRT_WF_TAIL_ROUND"]
        print(f"{scene} {W}x{H} {spp}spp  default, no tail kernel  {t * 1e3:7.1f} ms", flush=True)
        n_eq, t = spp * times[False] / times[True], times[True]
        for _ in range(3):
            n_try = max(1, int(round(n_eq)))
            p = api.default_params(W, H, n_try, nee=True)
            (img, _), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), a.reps)
            n_eq = n_try * times[False] / t
        print(f"{scene} {W}x{H} {n_try}spp  nee (equal time)  {t * 1e3:7.1f} ms (default {times[False] * 1e3:.1f} ms)  rms {rms(img):.5g}", flush=True)
        dev.close()


if __name__ == "__main__":
    main()
