"""Adaptive sampling against the uniform render (include/hrt.h hrt_render_stripes_adaptive): for the headline frame
(teapot_scene.yaml 640x640, 100 spp, the bench's stand-in assets) and cornell_box.yaml (256x256, 256 spp) prints, per threshold,
the samples taken, their share of the uniform render's, the frame time (host wall clock around all passes, best of `--reps`;
`host` = DeviceScene.render_adaptive on host buffers, `dev` = hrt_render_stripes_adaptive_device + hrt_adaptive_mean_device on
torch device buffers, one 4-byte read-back per pass),
and the RMS error of the linear film against a high-spp uniform render (`--ref-mult` x spp, seed 1: independent of the films
compared).  The uniform render at the same spp is the first line of each scene.
  python3 tests/tools/adaptive_time.py [--thresholds 0.02,0.05,0.1,0.2] [--pass-samples 16,32] [--reps 3] [--ref-mult 8]"""
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


def run_device(dev, cam, p, ad, W, H):
    import torch
    sums = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    sq = torch.empty((H, W), dtype=torch.float32, device="cuda")
    count = torch.empty((H, W), dtype=torch.int32, device="cuda")
    mean = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    k = 0
    while dev.render_stripes_adaptive_device(cam, p, 8, 0, 1, ad, sums.data_ptr(), sq.data_ptr(), count.data_ptr(), k, s):
        k += 1
    dev.adaptive_mean_device(sums.data_ptr(), count.data_ptr(), W * H, mean.data_ptr(), s)
    torch.cuda.synchronize()
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--thresholds", default="0.02,0.05,0.1,0.2")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-mult", type=int, default=8)
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--pass-samples", default="16", help="comma-separated: one row per value")
    ap.add_argument("--floor", type=float, default=0.01)
    a = ap.parse_args()
    d = tempfile.mkdtemp()
    api.write_teapot_obj(os.path.join(d, "teapot.obj"), 1.0)
    api.write_hall_hdr(os.path.join(d, "old_hall_4k.hdr"), 4096, 2048)
    for scene, W, H, spp in (("teapot_scene.yaml", 640, 640, 100), ("cornell_box.yaml", 256, 256, 256)):
        hs = api.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", scene), d)
        dev = api.DeviceScene(hs.flat_ptr, 0)
        cam, p = hs.camera(W, H), api.default_params(W, H, spp)
        ref, _ = dev.render_stripes(cam, api.default_params(W, H, spp * a.ref_mult, seed=1), 8, 0, 1)
        ref = ref.astype(np.float64)
        rms = lambda img: float(np.sqrt(np.mean((img.astype(np.float64) - ref) ** 2)))   # noqa: E731
        dev.render_stripes(cam, p, 8, 0, 1)
        (uni, _), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), a.reps)
        n_uni = W * H * spp
        print(f"{scene} {W}x{H} {spp}spp  uniform                    samples {n_uni:>11d}  1.000  {t * 1e3:6.1f} ms  rms {rms(uni):.5g}")
        for ps in (int(x) for x in a.pass_samples.split(",")):
            for thr in (float(x) for x in a.thresholds.split(",")):
                ad = api.Adaptive(min(a.min_samples, spp), ps, thr, a.floor)
                (mean, count, st), t = best(lambda: dev.render_adaptive(cam, p, ad), a.reps)
                passes, td = best(lambda: run_device(dev, cam, p, ad, W, H), a.reps)
                n = int(count.sum())
                print(f"{scene} {W}x{H} {spp}spp  adaptive {thr:<6g} pass {ps:<3d} samples {n:>11d}  {n / n_uni:.3f}  host {t * 1e3:6.1f} ms"
                      f"  dev {td * 1e3:6.1f} ms ({passes} passes)  rms {rms(mean):.5g}")
        dev.close()


if __name__ == "__main__":
    main()
