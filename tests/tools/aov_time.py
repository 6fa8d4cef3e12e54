"""What the feature-buffer pass (hrt_render_aov_stripes_device) costs on the headline frame: teapot_scene.yaml, 640 x 640,
the bench's stand-in assets.  HIP events around the call only, on the stream the call is given; best of `--reps` after `--warmup`:
the pass at 16 and at 100 samples per pixel, philox and stratified, and the film's own frame (hrt_render_stripes_device, 100 spp) the
same way.  Prints one JSON line (DESIGN.md 4.11 quotes it).
  python3 tests/tools/aov_time.py [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from hobbyraytracer_amd import api  # noqa: E402

W = H = 640
SPP = 100


def best_ms(call, reps, warmup):
    stream = torch.cuda.current_stream()
    times = []
    for k in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call(stream.cuda_stream)
        b.record(stream)
        b.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b))
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        print(json.dumps(measure(d, args.reps, args.warmup)))


def measure(d, reps, warmup):
    api.write_teapot_obj(os.path.join(d, "teapot.obj"), 1.0)
    api.write_hall_hdr(os.path.join(d, "old_hall_4k.hdr"), 4096, 2048)
    hs = api.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", "teapot_scene.yaml"), d)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    cam = hs.camera(W, H)
    aov = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
    film = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out = {"frame": f"teapot_scene {W}x{H}", "reps": reps, "warmup": warmup}
    for n in (16, SPP):
        for name, strat in (("", False), ("_stratified", True)):
            p = api.default_params(W, H, n, stratified=strat)
            out[f"aov_{n}spp{name}_ms"] = round(best_ms(lambda s: dev.render_aov_stripes_device(cam, p, 8, 0, 1, aov.data_ptr(), 0, -1, s), reps, warmup), 4)
    p = api.default_params(W, H, SPP)
    out["beauty_100spp_ms"] = round(best_ms(lambda s: dev.render_stripes_device(cam, p, 8, 0, 1, film.data_ptr(), s), reps, warmup), 4)
    out["aov_16_over_beauty"] = round(out["aov_16spp_ms"] / out["beauty_100spp_ms"], 5)
    out["aov_100_over_beauty"] = round(out["aov_100spp_ms"] / out["beauty_100spp_ms"], 5)
    alpha = aov[..., 3]
    out["coverage"] = round(float(alpha.mean()), 5)
    dev.stats()                       # folds the film renders' events
    dev.close()
    return out


if __name__ == "__main__":
    main()
