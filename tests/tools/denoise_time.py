"""What the guided denoiser (hrt_denoise_device) costs on the headline frame: teapot_scene.yaml, 640 x 640, the bench's
stand-in assets, the film at 100 samples per pixel and its feature buffers at 16.  HIP events around hrt_denoise_device only, on the
stream the call is given; best of `--reps` after `--warmup`; default parameters; with a given variance and with the spatial estimate;
and with one iteration, so that the cost of an iteration is (default - one) / (iterations - 1).  The yardstick printed beside it is the
compulsory traffic of one iteration -- 64 bytes per pixel, its two float4 read once and written once -- at the HBM rate a streaming kernel
achieves on this part (--hbm-gbps, 6300 by default: the rate a float4 copy reaches).  Prints one JSON line (DESIGN.md 4.12 quotes it).
  python3 tests/tools/denoise_time.py [--reps 5] [--warmup 2]"""
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
SPP, AOV_SPP = 100, 16


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
    film = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    aov = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    ws = torch.empty(api.denoise_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    dev.render_stripes_device(cam, api.default_params(W, H, SPP), 8, 0, 1, film.data_ptr(), 0)
    dev.render_aov_stripes_device(cam, api.default_params(W, H, AOV_SPP), 8, 0, 1, aov.data_ptr(), 0, -1, 0)
    torch.cuda.synchronize()
    # a stand-in for the adaptive buffers' variance: its values do not change what the kernels execute
    lum = 0.2126 * film[..., 0] + 0.7152 * film[..., 1] + 0.0722 * film[..., 2]
    var = (0.05 * lum * lum / SPP).contiguous()
    torch.cuda.synchronize()
    p = api.denoise_defaults()
    one = api.denoise_defaults(iterations=1)
    res = {"frame": f"teapot_scene {W}x{H}", "film_spp": SPP, "aov_spp": AOV_SPP, "reps": reps, "warmup": warmup, "iterations": p.iterations}

    def call(params, v):
        return lambda s: api.denoise_device(W, H, film.data_ptr(), aov.data_ptr(), out.data_ptr(), ws.data_ptr(), v, stream=s, params=params)
    res["denoise_var_ms"] = round(best_ms(call(p, var.data_ptr()), reps, warmup), 4)
    res["denoise_spatial_ms"] = round(best_ms(call(p, None), reps, warmup), 4)
    res["denoise_var_1_iteration_ms"] = round(best_ms(call(one, var.data_ptr()), reps, warmup), 4)
    res["denoise_spatial_1_iteration_ms"] = round(best_ms(call(one, None), reps, warmup), 4)
    res["per_iteration_ms"] = round((res["denoise_var_ms"] - res["denoise_var_1_iteration_ms"]) / (p.iterations - 1), 4)
    res["spatial_variance_ms"] = round(res["denoise_spatial_1_iteration_ms"] - res["denoise_var_1_iteration_ms"], 4)
    res["iteration_floor_ms"] = round(64.0 * W * H / (hbm_gbps * 1e9) * 1e3, 4)        # 64 B per pixel at the achievable HBM rate
    res["floor_over_iteration"] = round(res["iteration_floor_ms"] / res["per_iteration_ms"], 4) if res["per_iteration_ms"] > 0 else None
    pf = api.default_params(W, H, SPP)
    res["beauty_100spp_ms"] = round(best_ms(lambda s: dev.render_stripes_device(cam, pf, 8, 0, 1, film.data_ptr(), s), reps, warmup), 4)
    res["denoise_over_beauty"] = round(res["denoise_spatial_ms"] / res["beauty_100spp_ms"], 5)
    res["changed_pixels"] = round(float((out != film).any(dim=-1).float().mean()), 5)
    dev.stats()                       # folds the film renders' events
    dev.close()
    return res


if __name__ == "__main__":
    main()
