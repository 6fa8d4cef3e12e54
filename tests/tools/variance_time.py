"""What the measured variance (hrt_variance_*) costs on the headline frame: teapot_scene.yaml, 640 x 640, the bench's
stand-in assets, 100 samples per pixel.  Two things, in one session on one build.
(1) The kernels: HIP events around one hrt_variance_fold_device + one hrt_variance_finish_device (and around each alone), on the stream the
calls are given; best of `--reps` after `--warmup`.  The yardstick printed beside it is their compulsory traffic -- a fold reads 12 + 8
and writes 8 bytes per pixel, the finish reads 8 and writes 4 -- at the HBM rate a streaming kernel achieves on this part (--hbm-gbps, 6300
by default: the rate DESIGN.md 4.12 uses).
(2) The batching: the frame through hrt_render_stripes_accumulate_device in 1, 2, 4 and 8 passes (the ranges of api.variance_batches), HIP
events around all passes of a frame, without and with the folds in between; every pass repeats the late rounds of the wavefront pipeline,
in which few paths are left, so K passes are not free.  Prints one JSON line (DESIGN.md 4.13 quotes it).
  python3 tests/tools/variance_time.py [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from hobbyraytracer_amd import api  # noqa: E402
from tests.tools.denoise_time import best_ms  # noqa: E402

W = H = 640
SPP = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hbm-gbps", type=float, default=6300.0)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        print(json.dumps(measure(d, args.reps, args.warmup, args.hbm_gbps)))


def measure(d, reps, warmup, hbm_gbps):
    api.write_teapot_obj(os.path.join(d, "teapot.obj"), 1.0)
    api.write_hall_hdr(os.path.join(d, "old_hall_4k.hdr"), 4096, 2048)
    hs = api.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", "teapot_scene.yaml"), d)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    cam = hs.camera(W, H)
    n = W * H
    p = api.default_params(W, H, SPP)
    film = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    state = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    var = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    dev.render_stripes_accumulate_device(cam, p, 8, 0, 1, film.data_ptr(), 0, SPP // 2, 0)
    api.variance_fold_device(n, film.data_ptr(), 0, SPP // 2, state.data_ptr())
    torch.cuda.synchronize()
    res = {"frame": f"teapot_scene {W}x{H}", "spp": SPP, "reps": reps, "warmup": warmup}

    def fold(s):
        api.variance_fold_device(n, film.data_ptr(), SPP // 2, SPP // 2, state.data_ptr(), stream=s)

    def finish(s):
        api.variance_finish_device(n, state.data_ptr(), SPP, 2, var.data_ptr(), stream=s)
    res["fold_ms"] = round(best_ms(fold, reps, warmup), 5)
    res["finish_ms"] = round(best_ms(finish, reps, warmup), 5)
    res["fold_and_finish_ms"] = round(best_ms(lambda s: (fold(s), finish(s)), reps, warmup), 5)
    res["fold_floor_ms"] = round(28.0 * n / (hbm_gbps * 1e9) * 1e3, 5)                 # 12 + 8 read, 8 written per pixel
    res["finish_floor_ms"] = round(12.0 * n / (hbm_gbps * 1e9) * 1e3, 5)               # 8 read, 4 written per pixel
    res["floor_over_fold_and_finish"] = round((res["fold_floor_ms"] + res["finish_floor_ms"]) / res["fold_and_finish_ms"], 4)

    def frame(batches, with_folds):
        ranges = api.variance_batches(SPP, batches)

        def call(s):
            for first, count in ranges:
                dev.render_stripes_accumulate_device(cam, p, 8, 0, 1, film.data_ptr(), first, count, s)
                if with_folds:
                    api.variance_fold_device(n, film.data_ptr(), first, count, state.data_ptr(), scale=float(SPP) if first + count == SPP else 1.0, stream=s)
            if with_folds:
                api.variance_finish_device(n, state.data_ptr(), SPP, len(ranges), var.data_ptr(), stream=s)
        return call
    for k in (1, 2, 4, 8):
        res[f"frame_{k}_passes_ms"] = round(best_ms(frame(k, False), reps, warmup), 4)
    for k in (2, 4, 8):
        res[f"frame_{k}_passes_with_variance_ms"] = round(best_ms(frame(k, True), reps, warmup), 4)
        res[f"passes_{k}_over_1"] = round(res[f"frame_{k}_passes_ms"] / res["frame_1_passes_ms"], 4)
        res[f"passes_{k}_with_variance_over_1"] = round(res[f"frame_{k}_passes_with_variance_ms"] / res["frame_1_passes_ms"], 4)
    res["variance_pixels_positive"] = round(float((var > 0).float().mean()), 5)
    dev.stats()                       # folds the film renders' events
    dev.close()
    return res


if __name__ == "__main__":
    main()
