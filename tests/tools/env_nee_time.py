"""Environment-map sampling (HRT_FLAG_NEE_ENV) against --nee and the default estimator: for the headline frame
(teapot_scene.yaml 640x640, 100 spp, the bench's stand-in assets) and tests/test_gpu_env_nee.py's env_scene (256x256, 64 spp) prints the
frame time (host wall clock around hrt_render_stripes, best of `--reps`), the path segments, the shadow rays and the RMS error of the
linear film against a high-spp reference (`--ref-mult` x spp, seed 1, the mean of the three estimators' films).  Then equal-time rows:
--nee and --nee-env at the sample counts whose measured times match the default render's.  Also the time of hrt_env_table_build on the
4096 x 2048 hall map (with its copies); hrt_scene_create, which builds the table, is timed by tests/tools/scene_create_time.py.
  python3 tests/tools/env_nee_time.py [--reps 3] [--ref-mult 8]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from hobbyraytracer_amd import api  # noqa: E402
from tests.test_gpu_env_nee import ENV_SCENE_YAML  # noqa: E402

MODES = {"default": {}, "nee": {"nee": True}, "nee-env": {"nee_env": True}}


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
    hall = api.read_hdr(os.path.join(d, "old_hall_4k.hdr"))
    api.env_table_build(hall)
    _, t = best(lambda: api.env_table_build(hall), a.reps)
    print(f"hrt_env_table_build 4096x2048 (upload + build + download): {t * 1e3:.2f} ms", flush=True)
    with open(os.path.join(d, "env_scene.yaml"), "w") as f:
        f.write(ENV_SCENE_YAML)
    for path, W, H, spp in ((os.path.join(ROOT, "tests", "golden", "scenes", "teapot_scene.yaml"), 640, 640, 100),
                            (os.path.join(d, "env_scene.yaml"), 256, 256, 64)):
        scene = os.path.basename(path)
        hs = api.HostScene(path, d)
        dev = api.DeviceScene(hs.flat_ptr, 0)
        cam = hs.camera(W, H)
        ref = np.zeros((H, W, 3))
        for kw in MODES.values():
            img, _ = dev.render_stripes(cam, api.default_params(W, H, spp * a.ref_mult, seed=1, **kw), 8, 0, 1)
            ref += img.astype(np.float64) / len(MODES)
        rms = lambda img: float(np.sqrt(np.mean((img.astype(np.float64) - ref) ** 2)))   # noqa: E731
        times = {}
        for name, kw in MODES.items():
            p = api.default_params(W, H, spp, **kw)
            dev.render_stripes(cam, p, 8, 0, 1)
            (img, st), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), a.reps)
            times[name] = t
            print(f"{scene} {W}x{H} {spp}spp  {name:8s} {t * 1e3:8.1f} ms  rays {st.rays:>12d}  shadow_rays {st.shadow_rays:>12d}"
                  f"  rms {rms(img):.5g}", flush=True)
        for name in ("nee", "nee-env"):   # equal time: correct the sample count twice from what was measured
            n_eq, t = spp * times["default"] / times[name], times[name]
            for _ in range(3):
                n_try = max(1, int(round(n_eq)))
                p = api.default_params(W, H, n_try, **MODES[name])
                (img, _), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), a.reps)
                n_eq = n_try * times["default"] / t
            print(f"{scene} {W}x{H} {n_try}spp  {name} (equal time)  {t * 1e3:.1f} ms (default {times['default'] * 1e3:.1f} ms)"
                  f"  rms {rms(img):.5g}", flush=True)
        dev.close()


if __name__ == "__main__":
    main()
