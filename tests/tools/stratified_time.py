"""The stratified sampler (HRT_FLAG_STRATIFIED) against the default one.

Time (the default mode): cornell_box.yaml (256x256, 256 spp) and the headline frame (teapot_scene.yaml 640x640, 100 spp, the bench's
stand-in assets), default and --nee, each with and without --stratified: host wall clock around hrt_render_stripes, best of `--reps`.
The flag renders round by round (no tail kernel), so the default render on that schedule (HRT_WF_TAIL_ROUND >= max_depth) is timed too:
that row, not the first, is what the sampler's own cost compares with.

Error (--error): r = RMS_stratified / RMS_default against the closed form on the floor scene of tests/test_gpu_stratified.py at 4, 16 and
64 spp over the seeds 0..7, the spread of r at 16 spp over 8 disjoint groups of 8 seeds, and r on cornell_box.yaml 64x64 at 16 spp with
and without --nee against a 2048-spp mean of both samplers' films (other seeds).
  python3 tests/tools/stratified_time.py [--reps 3] [--error]"""
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


def timing(reps):
    d = tempfile.mkdtemp()
    api.write_teapot_obj(os.path.join(d, "teapot.obj"), 1.0)
    api.write_hall_hdr(os.path.join(d, "old_hall_4k.hdr"), 4096, 2048)
    for scene, W, H, spp in (("cornell_box.yaml", 256, 256, 256), ("teapot_scene.yaml", 640, 640, 100)):
        hs = api.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", scene), d)
        dev = api.DeviceScene(hs.flat_ptr, 0)
        cam = hs.camera(W, H)
        for nee in (False, True):
            for strat, no_tail in ((False, False), (False, True), (True, False)):
                if no_tail and nee:
                    continue          # --nee already renders round by round
                if no_tail:
                    os.environ["HRT_WF_TAIL_ROUND"] = "1000000"
                p = api.default_params(W, H, spp, nee=nee, stratified=strat)
                dev.render_stripes(cam, p, 8, 0, 1)
                (img, st), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), reps)
                os.environ.pop("HRT_WF_TAIL_ROUND", None)
                what = ("nee" if nee else "default") + (" stratified" if strat else "") + (", no tail kernel" if no_tail else "")
                print(f"{scene} {W}x{H} {spp}spp  {what:<28s}  {t * 1e3:7.1f} ms  rays {st.rays:>12d}  shadow_rays {st.shadow_rays:>12d}", flush=True)
        dev.close()


def error():
    from tests import test_gpu_stratified as T
    d = tempfile.mkdtemp()
    hs = T._scene(d, "floor", T.FLOOR_YAML)
    W = H = 64
    cam = hs.camera(W, H)
    pred = T.floor_prediction(cam, W, H)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    for spp in (4, 16, 64):
        a = T.floor_rms(api, dev, cam, pred, W, H, spp, range(8), False)
        b = T.floor_rms(api, dev, cam, pred, W, H, spp, range(8), True)
        print(f"floor {spp} spp seeds 0..7: relative RMS default {a:.5f}, stratified {b:.5f}, r = {b / a:.4f}", flush=True)
    rs = []
    for g in range(8):
        seeds = range(8 * g, 8 * g + 8)
        rs.append(T.floor_rms(api, dev, cam, pred, W, H, 16, seeds, True) / T.floor_rms(api, dev, cam, pred, W, H, 16, seeds, False))
    print("floor 16 spp, r of 8 disjoint seed groups: " + " ".join(f"{r:.4f}" for r in rs) + f"; mean {np.mean(rs):.4f}, std {np.std(rs, ddof=1):.4f}", flush=True)
    dev.close()
    api.write_teapot_obj(os.path.join(d, "teapot.obj"), 1.0)
    hs = api.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", "cornell_box.yaml"), d)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    cam = hs.camera(W, H)
    for nee in (False, True):
        a, b = T.cornell_ratio(api, dev, cam, W, H, nee)
        print(f"cornell_box 64x64 16 spp nee={nee}: RMS vs 2048-spp mean of both samplers: default {a:.5f}, stratified {b:.5f}, r = {b / a:.4f}", flush=True)
    dev.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--error", action="store_true")
    a = ap.parse_args()
    error() if a.error else timing(a.reps)
