"""What the outlier filter (hrt_despeckle_device) costs on the headline frame: teapot_scene.yaml, 640 x 640, the bench's
stand-in assets, the film at 16 samples per pixel (where people denoise) with its measured variance.  HIP events around
hrt_despeckle_device only, on the stream the call is given; best of `--reps` after `--warmup`; default parameters and the largest window;
with and without the variance and the map; hrt_denoise_device (default parameters, the same film and variance) beside it in the same
run.  The yardstick printed beside it is the pass's compulsory traffic -- 12 bytes per pixel of film read and 12 written, plus its
20-byte workspace written once and read once: 64 bytes per pixel -- at the HBM rate a streaming kernel achieves on this part (--hbm-gbps,
6300 by default: the rate a float4 copy reaches).  Prints one JSON line (DESIGN.md 4.15 quotes it).
  python3 tests/tools/despeckle_time.py [--reps 5] [--warmup 2]"""
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
SPP, AOV_SPP = 16, 16


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
    film_np, var_np = dev.render_stripes_with_variance(cam, api.default_params(W, H, SPP), batches=4)
    film, var = torch.from_numpy(film_np).cuda(), torch.from_numpy(var_np).cuda()
    aov = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    dmap = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    ws = torch.empty(api.despeckle_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    dn_ws = torch.empty(api.denoise_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    dev.render_aov_stripes_device(cam, api.default_params(W, H, AOV_SPP), 8, 0, 1, aov.data_ptr(), 0, -1, 0)
    torch.cuda.synchronize()
    p, wide = api.despeckle_defaults(), api.despeckle_defaults(radius=2, rank=4)
    res = {"frame": f"teapot_scene {W}x{H}", "film_spp": SPP, "reps": reps, "warmup": warmup}

    def call(params, v, m):
        return lambda s: api.despeckle_device(W, H, film.data_ptr(), out.data_ptr(), ws.data_ptr(), v, m, stream=s, params=params)
    res["despeckle_ms"] = round(best_ms(call(p, None, None), reps, warmup), 4)
    res["despeckle_var_map_ms"] = round(best_ms(call(p, var.data_ptr(), dmap.data_ptr()), reps, warmup), 4)
    torch.cuda.synchronize()
    res["outliers_gated"] = int((dmap > 0).sum())
    res["despeckle_5x5_rank4_ms"] = round(best_ms(call(wide, None, dmap.data_ptr()), reps, warmup), 4)
    best_ms(call(p, None, dmap.data_ptr()), 1, 0)
    torch.cuda.synchronize()
    res["outliers"] = int((dmap > 0).sum())
    res["changed_pixels"] = round(float((out != film).any(dim=-1).float().mean()), 5)
    res["luminance_kept"] = round(float(out.double().sum() / film.double().sum()), 9)
    res["floor_ms"] = round(64.0 * W * H / (hbm_gbps * 1e9) * 1e3, 4)                # 64 B per pixel at the achievable HBM rate
    res["floor_over_despeckle"] = round(res["floor_ms"] / res["despeckle_ms"], 4)
    dn = api.denoise_defaults()
    res["denoise_var_ms"] = round(best_ms(lambda s: api.denoise_device(W, H, film.data_ptr(), aov.data_ptr(), out.data_ptr(), dn_ws.data_ptr(), var.data_ptr(),
                                                                         stream=s, params=dn), reps, warmup), 4)
    res["denoise_spatial_ms"] = round(best_ms(lambda s: api.denoise_device(W, H, film.data_ptr(), aov.data_ptr(), out.data_ptr(), dn_ws.data_ptr(), None,
                                                                             stream=s, params=dn), reps, warmup), 4)
    res["despeckle_over_denoise"] = round(res["despeckle_ms"] / res["denoise_spatial_ms"], 4)
    dev.stats()                       # folds the film render's events
    dev.close()
    return res


if __name__ == "__main__":
    main()
