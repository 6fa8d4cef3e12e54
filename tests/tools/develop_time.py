"""What the develop stage (hrt_develop_device) costs: a seeded synthetic film (log-normal luminances over about ten stops,
a few small lights) of 640 x 640 and of 2048 x 2048, 5 levels at the default strength and auto exposure.  HIP events around
hrt_develop_device only, on the stream the call is given; the median of `--reps` (at least 20) after `--warmup`.  Beside the whole stage,
the calls that leave parts of it out (no bloom; no meter; neither: the write kernel alone; one level), from which the cost of a part is
read as a difference, and the launches each makes; per-kernel times come from a kernel trace of this script, in a run of its own.
hrt_despeckle_device and hrt_denoise_device (default parameters, a zero feature buffer) run on the same films in the same session.  The
yardstick printed beside it is the stage's own traffic, counted from the level sizes, at the rate of the memory level the film and its
pyramid sit in between two launches (--cache-gbps, 8600 by default: the Infinity Cache; a 2048 x 2048 film and its pyramid are 74 MB).
Prints one JSON line per film (DESIGN.md 4.17 quotes them).
  python3 tests/tools/develop_time.py [--reps 20] [--warmup 5] [--sizes 640,2048]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hobbyraytracer_amd import api  # noqa: E402

LEVELS = 5


def median_ms(call, reps, warmup):
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
    return statistics.median(times)


def film_of(side, seed=1):
    r = np.random.default_rng(seed)
    lum = np.exp2(r.normal(-3.0, 1.7, (side, side, 1))).astype(np.float32)
    film = lum * r.uniform(0.6, 1.0, (side, side, 3)).astype(np.float32)
    for _ in range(6):                                              # small lights
        y, x = r.integers(8, side - 16, 2)
        film[y:y + 6, x:x + 6] = 12.0
    return film


def traffic_bytes(W, H, levels):
    """what the launches of a call with `levels` levels and auto exposure read and write, from the level sizes"""
    n = W * H
    sizes, w, h = [], W, H
    for _ in range(levels):
        if max(w, h) <= 1:
            break
        w, h = (w + 1) // 2, (h + 1) // 2
        sizes.append(w * h)
    total = 0
    if sizes:
        total += 12 * n + 16 * sizes[0]                             # k_dv_down_film
        for a, b in zip(sizes, sizes[1:]):
            total += 16 * a + 16 * b                                # k_dv_down
        for a, b in zip(sizes, sizes[1:]):
            total += 16 * b + 2 * 16 * a                            # k_dv_up_add: the coarse level, and the fine one read and written
    e1 = 16 * sizes[0] if sizes else 0
    total += 12 * n + e1                                            # k_dv_meter_film
    total += 12 * n + e1 + 12 * n                                   # k_dv_write
    return total


def launches(levels_effective, bloom, meter):
    return (2 * levels_effective - 1 if bloom and levels_effective else 0) + (3 if meter else 0) + 1      # (the counters' clear is one)


def measure(side, reps, warmup, cache_gbps):
    W = H = side
    film = torch.from_numpy(film_of(side)).cuda()
    out = torch.zeros_like(film)
    ws = torch.empty(api.develop_workspace_bytes(W, H, LEVELS), dtype=torch.uint8, device="cuda")
    info = torch.zeros(3, dtype=torch.int64, device="cuda")
    res = {"film": f"synthetic {W}x{H}", "levels": LEVELS, "reps": reps, "warmup": warmup}

    def call(**kw):
        p = api.develop_defaults(**kw)
        return lambda s: api.develop_device(W, H, film.data_ptr(), out.data_ptr(), ws.data_ptr(), stream=s, params=p)
    res["stage_ms"] = round(median_ms(call(bloom_levels=LEVELS, exposure_mode=2), reps, warmup), 4)
    res["stage_launches"] = launches(LEVELS, True, True)
    res["bloom_only_ms"] = round(median_ms(call(bloom_levels=LEVELS), reps, warmup), 4)
    res["bloom_only_launches"] = launches(LEVELS, True, False)
    res["one_level_ms"] = round(median_ms(call(bloom_levels=1), reps, warmup), 4)
    res["meter_only_ms"] = round(median_ms(call(exposure_mode=2), reps, warmup), 4)
    res["write_only_ms"] = round(median_ms(call(exposure_mode=1, exposure_ev=1.0), reps, warmup), 4)
    res["in_place_ms"] = round(median_ms(lambda s: api.develop_device(W, H, out.data_ptr(), out.data_ptr(), ws.data_ptr(), stream=s,
                                                                      params=api.develop_defaults(bloom_levels=LEVELS, exposure_mode=2)), reps, warmup), 4)
    api.develop_device(W, H, film.data_ptr(), out.data_ptr(), ws.data_ptr(), info.data_ptr(), params=api.develop_defaults(bloom_levels=LEVELS, exposure_mode=2))
    torch.cuda.synchronize()
    got = api.DevelopInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    res["scale"], res["mean_ev"], res["metered"] = round(got.scale, 6), round(got.mean_ev, 6), got.metered
    res["bytes"] = traffic_bytes(W, H, LEVELS)
    res["bytes_per_pixel"] = round(res["bytes"] / (W * H), 2)
    res["floor_ms"] = round(res["bytes"] / (cache_gbps * 1e9) * 1e3, 4)
    res["floor_over_stage"] = round(res["floor_ms"] / res["stage_ms"], 4)
    res["us_per_launch"] = round(1e3 * res["stage_ms"] / res["stage_launches"], 3)
    # the two cleaning stages on the same film
    ds_ws = torch.empty(api.despeckle_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    dn_ws = torch.empty(api.denoise_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    aov = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
    ds, dn = api.despeckle_defaults(), api.denoise_defaults()
    res["despeckle_ms"] = round(median_ms(lambda s: api.despeckle_device(W, H, film.data_ptr(), out.data_ptr(), ds_ws.data_ptr(), stream=s, params=ds), reps, warmup), 4)
    res["denoise_spatial_ms"] = round(median_ms(lambda s: api.denoise_device(W, H, film.data_ptr(), aov.data_ptr(), out.data_ptr(), dn_ws.data_ptr(), None,
                                                                               stream=s, params=dn), reps, warmup), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="640,2048")
    ap.add_argument("--cache-gbps", type=float, default=8600.0)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20: the figure is a median")
    for side in (int(v) for v in args.sizes.split(",")):
        print(json.dumps(measure(side, args.reps, args.warmup, args.cache_gbps)), flush=True)


if __name__ == "__main__":
    main()
