"""What the id-matte pass (hrt_render_aov_ids_stripes_device) costs on the headline frame: teapot_scene.yaml, 640 x 640,
the bench's stand-in assets.  HIP events around the device-pointer call only, on the stream the call is given; best of `--reps` after
`--warmup`: the pass at 16 and at 100 samples per pixel, and in the same session the feature-buffer pass
(hrt_render_aov_stripes_device) at the same counts and the film's own frame (hrt_render_stripes_device, 100 spp).  Prints one JSON
line (DESIGN.md 4.14 quotes it).
  python3 tests/tools/aov_ids_time.py [--reps 5] [--warmup 2]"""
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
from tests.tools.aov_time import H, SPP, W, best_ms  # noqa: E402


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
    ids = torch.zeros((api.aov_ids_bytes(W * H) // 4,), dtype=torch.float32, device="cuda")
    aov = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
    film = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out = {"frame": f"teapot_scene {W}x{H}", "reps": reps, "warmup": warmup}
    for n in (16, SPP):
        p = api.default_params(W, H, n)
        out[f"ids_{n}spp_ms"] = round(best_ms(lambda s: dev.render_aov_ids_stripes_device(cam, p, 8, 0, 1, ids.data_ptr(), 0, -1, s), reps, warmup), 4)
        out[f"aov_{n}spp_ms"] = round(best_ms(lambda s: dev.render_aov_stripes_device(cam, p, 8, 0, 1, aov.data_ptr(), 0, -1, s), reps, warmup), 4)
        out[f"ids_over_aov_{n}spp"] = round(out[f"ids_{n}spp_ms"] / out[f"aov_{n}spp_ms"], 4)
    p = api.default_params(W, H, SPP, stratified=True)
    out["ids_100spp_stratified_ms"] = round(best_ms(lambda s: dev.render_aov_ids_stripes_device(cam, p, 8, 0, 1, ids.data_ptr(), 0, -1, s), reps, warmup), 4)
    p = api.default_params(W, H, SPP)
    out["beauty_100spp_ms"] = round(best_ms(lambda s: dev.render_stripes_device(cam, p, 8, 0, 1, film.data_ptr(), s), reps, warmup), 4)
    out["ids_100_over_beauty"] = round(out["ids_100spp_ms"] / out["beauty_100spp_ms"], 5)
    buf = ids.cpu().numpy().view(api.AOV_IDS_DTYPE).reshape(H, W)       # (the stratified call's, 100 spp)
    out["pixels_with_two_or_more_objects"] = round(float((buf["object_id"][..., 1] != api.AOV_ID_UNUSED).mean()), 5)
    out["pixels_with_five_or_more_objects"] = round(float((np.rint(buf["object_coverage"].astype(np.float64).sum(axis=-1) * SPP) < SPP).mean()), 5)
    dev.stats()                       # folds the film renders' events
    dev.close()
    return out


if __name__ == "__main__":
    main()
