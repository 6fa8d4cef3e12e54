"""Next-event estimation over the emitter table (HRT_FLAG_NEE_EMITTERS) against the default estimator and --nee: for the
emissive-teapot scene of tests/test_gpu_nee_emitters.py and cornell_box.yaml with its lamp under rotate_y (256x256, 64 spp) prints the
frame time (host wall clock around hrt_render_stripes, best of `--reps`), the path segments, the shadow rays and the RMS error of the
linear film against a high-spp reference (`--ref-mult` x spp, seed 1, the mean of the default and the emitter films).  Then an equal-time
row: --nee-emitters at the sample count whose measured time matches the default render's.
  python3 tests/tools/nee_emitters_time.py [--reps 3] [--ref-mult 8]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from hobbyraytracer_amd import api  # noqa: E402
from tests.test_gpu_nee_emitters import TEAPOT_LAMP_YAML, _rotated_cornell  # noqa: E402

MODES = {"default": {}, "nee": {"nee": True}, "emitters": {"nee_emitters": True}}


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
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    d = tempfile.mkdtemp()
    api.write_teapot_obj(os.path.join(d, "teapot.obj"), 1.0)
    W = H = a.size
    spp = a.spp
    for name, yaml in (("teapot_lamp", TEAPOT_LAMP_YAML), ("rotated_cornell", _rotated_cornell(os.path.join(ROOT, "tests", "golden", "scenes")))):
        path = os.path.join(d, name + ".yaml")
        with open(path, "w") as f:
            f.write(yaml)
        hs = api.HostScene(path, d)
        dev = api.DeviceScene(hs.flat_ptr, 0)
        cam = hs.camera(W, H)
        ref = np.zeros((H, W, 3))
        for kw in (MODES["default"], MODES["emitters"]):
            img, _ = dev.render_stripes(cam, api.default_params(W, H, spp * a.ref_mult, seed=1, **kw), 8, 0, 1)
            ref += 0.5 * img.astype(np.float64)
        rms = lambda img: float(np.sqrt(np.mean((img.astype(np.float64) - ref) ** 2)))   # noqa: E731
        times = {}
        for mode, kw in MODES.items():
            p = api.default_params(W, H, spp, **kw)
            dev.render_stripes(cam, p, 8, 0, 1)
            (img, st), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), a.reps)
            times[mode] = t
            print(f"{name} {W}x{H} {spp}spp  {mode:8s} {t * 1e3:8.1f} ms  rays {st.rays:>11d}  shadow_rays {st.shadow_rays:>11d}"
                  f"  rms {rms(img):.5g}", flush=True)
        n_eq = spp * times["default"] / times["emitters"]
        for _ in range(3):
            n_try = max(1, int(round(n_eq)))
            p = api.default_params(W, H, n_try, nee_emitters=True)
            (img, _), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), a.reps)
            n_eq = n_try * times["default"] / t
        print(f"{name} {W}x{H} {n_try}spp  emitters (equal time)  {t * 1e3:.1f} ms (default {times['default'] * 1e3:.1f} ms)"
              f"  rms {rms(img):.5g}", flush=True)
        dev.close()


if __name__ == "__main__":
    main()
