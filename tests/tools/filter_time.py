"""What the reconstruction filter (HRT_FLAG_FILTER) costs on the headline frame: teapot_scene.yaml, 640 x 640, 100 samples
per pixel, the bench's stand-in assets.  HIP events around hrt_render_stripes_device, on the stream the call is given; best of `--reps`
after `--warmup`; each kind at its default radius against the unfiltered frame of the same build in the same session, the unfiltered
frame measured before and after them.  Beside each, the time of the filter's own kernels in that call (hrt_scene_filter_ms: HIP events
around the gather and the finishing kernel; k_wf_reduce's run into its private film is not in it), and the yardstick: the compulsory
traffic of reading every sample's radiance once -- 16 bytes per slot -- at the HBM rate a streaming kernel achieves on this part
(--hbm-gbps, 6300 by default: the rate a float4 copy reaches).  With --image-effect also DESIGN.md 4.16's table: cornell_box at
64 x 64 x 16 spp, each kind beside the box film.  Prints one JSON line per part.
  python3 tests/tools/filter_time.py [--reps 5] [--warmup 2] [--image-effect]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hobbyraytracer_amd import api  # noqa: E402

W = H = 640
SPP = 100
KINDS = ("tent", "bspline", "mitchell")


def best_ms(call, reps, warmup, after=None):
    """best event time of call(stream) and what after() returned in that repetition"""
    stream = torch.cuda.current_stream()
    best = None
    for k in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call(stream.cuda_stream)
        b.record(stream)
        b.synchronize()
        extra = after() if after else None
        if k >= warmup and (best is None or a.elapsed_time(b) < best[0]):
            best = (a.elapsed_time(b), extra)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hbm-gbps", type=float, default=6300.0)
    ap.add_argument("--image-effect", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        api.write_teapot_obj(os.path.join(d, "teapot.obj"), 1.0)
        api.write_hall_hdr(os.path.join(d, "old_hall_4k.hdr"), 4096, 2048)
        print(json.dumps(measure(d, args.reps, args.warmup, args.hbm_gbps)), flush=True)
        if args.image_effect:
            print(json.dumps(image_effect(d)), flush=True)


def measure(d, reps, warmup, hbm_gbps):
    hs = api.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", "teapot_scene.yaml"), d)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    cam = hs.camera(W, H)
    film = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    plain, filtered = api.default_params(W, H, SPP), api.default_params(W, H, SPP, filter=True)
    res = {"frame": f"teapot_scene {W}x{H}x{SPP}", "reps": reps, "warmup": warmup}

    def frame(p):
        return lambda s: dev.render_stripes_device(cam, p, 8, 0, 1, film.data_ptr(), s)
    res["unfiltered_ms"] = round(best_ms(frame(plain), reps, warmup)[0], 4)
    for kind in KINDS:
        dev.set_filter(kind)
        dev.filter_ms()
        ms, own = best_ms(frame(filtered), reps, warmup, after=dev.filter_ms)
        res[f"{kind}_ms"] = round(ms, 4)
        res[f"{kind}_kernels_ms"] = round(own, 4)
    res["unfiltered_again_ms"] = round(best_ms(frame(plain), reps, warmup)[0], 4)
    res["read_rad_once_ms"] = round(16.0 * W * H * SPP / (hbm_gbps * 1e9) * 1e3, 4)
    dev.stats()                       # folds the renders' events
    dev.close()
    return res


def image_effect(d):
    """cornell_box 64 x 64 x 16 spp: every kind beside the box film.  Not an error against a converged film (that film is box-filtered
    itself): how far each film lies from the box film, how much of the box film's pixel-to-pixel roughness is left (the mean absolute
    difference between horizontal neighbours, of luminance), and the film's mean (a normalised filter keeps it but for the clamp)."""
    hs = api.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", "cornell_box.yaml"), d)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    w = h = 64
    cam = hs.camera(w, h)
    lum = lambda f: f.astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])      # noqa: E731
    rough = lambda f: float(np.abs(np.diff(lum(f), axis=1)).mean())               # noqa: E731
    box, _ = dev.render_tile(cam, api.default_params(w, h, 16, seed=1))
    res = {"frame": "cornell_box 64x64x16", "box": {"mean": round(float(lum(box).mean()), 5), "roughness": round(rough(box), 5)}}
    for kind in KINDS:
        dev.set_filter(kind)
        f, _ = dev.render_tile(cam, api.default_params(w, h, 16, seed=1, filter=True))
        res[kind] = {"mean": round(float(lum(f).mean()), 5), "roughness": round(rough(f), 5), "roughness_over_box": round(rough(f) / rough(box), 4),
                     "rms_from_box": round(float(np.sqrt(((f.astype(np.float64) - box) ** 2).mean())), 5), "negative_pixels": int((f < 0).sum())}
    dev.close()
    return res


if __name__ == "__main__":
    main()
