"""Russian roulette (HRT_FLAG_ROULETTE) against the default estimator.

Time (the default mode): cornell_box.yaml (256x256, 256 spp) and the headline frame (teapot_scene.yaml 640x640, 100 spp, the bench's
stand-in assets), each plain and with --nee, with and without --roulette: host wall clock around hrt_render_stripes, best of `--reps`.
The flag renders round by round (no tail kernel), so the plain render on that schedule (HRT_WF_TAIL_ROUND >= max_depth) is timed too.
  --other-tree DIR   every row WITHOUT the flag is timed again in child processes, alternating between the built tree DIR (a checkout
                     of the parent commit) and this one, to show that the default render did not move, to the segment.
Segments (--segments): st.rays with the flag / without it on cornell_box 256x256 64 spp --nee and the headline frame, seeds 0..7:
the ratio of seed 0, the mean and the seed-to-seed standard deviation, and the count without the flag
(tests/test_gpu_roulette.py SEGMENTS_MEASURED).
Error (--error): RMS error on cornell_box.yaml 128x128 --nee against the mean of both estimators' 2048-spp films (another seed), 8 seeds:
both at 64 spp, and roulette at the sample count that takes the default's time.
Frame (--frame [--roulette] [--nee]): renders the headline frame three times and nothing else -- the workload for
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tests/tools/roulette_time.py --frame --roulette
whose trace tests/tools/round_times.py turns into per-round times.
  python3 tests/tools/roulette_time.py [--reps 3] [--segments | --error | --frame]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.environ.get("HRT_ROULETTE_TIME_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (a child of --other-tree)
sys.path.insert(0, ROOT)
from hobbyraytracer_amd import api  # noqa: E402

CASES = (("cornell_box.yaml", 256, 256, 256), ("teapot_scene.yaml", 640, 640, 100))


def assets():
    d = tempfile.mkdtemp()
    api.write_teapot_obj(os.path.join(d, "teapot.obj"), 1.0)
    api.write_hall_hdr(os.path.join(d, "old_hall_4k.hdr"), 4096, 2048)
    return d


def scene(d, name):
    hs = api.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", name), d)
    return hs, api.DeviceScene(hs.flat_ptr, 0)


def best(fn, reps):
    out, t = None, float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t = min(t, time.perf_counter() - t0)
    return out, t


def rows_without_flag(reps):
    """{row name: best ms} of the renders that do not use the flag (what a build of the parent commit can render too)"""
    d = assets()
    out = {}
    for name, W, H, spp in CASES:
        hs, dev = scene(d, name)
        cam = hs.camera(W, H)
        for nee in (False, True):
            p = api.default_params(W, H, spp, nee=nee)
            dev.render_stripes(cam, p, 8, 0, 1)
            (_, st), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), reps)
            out[f"{name} {'nee' if nee else 'plain'}"] = (t * 1e3, st.rays)
        dev.close()
    return out


def timing(reps, other_tree):
    d = assets()
    for name, W, H, spp in CASES:
        hs, dev = scene(d, name)
        cam = hs.camera(W, H)
        for nee in (False, True):
            for rr, no_tail in ((False, False), (False, True), (True, False)):
                if no_tail and nee:
                    continue          # --nee already renders round by round
                if no_tail:
                    os.environ["HRT_WF_TAIL_ROUND"] = "1000000"
                p = api.default_params(W, H, spp, nee=nee, roulette=rr)
                dev.render_stripes(cam, p, 8, 0, 1)
                (_, st), t = best(lambda: dev.render_stripes(cam, p, 8, 0, 1), reps)
                os.environ.pop("HRT_WF_TAIL_ROUND", None)
                what = ("nee" if nee else "plain") + (" roulette" if rr else "") + (", no tail kernel" if no_tail else "")
                print(f"{name} {W}x{H} {spp}spp  {what:<28s}  {t * 1e3:7.1f} ms  rays {st.rays:>12d}  shadow_rays {st.shadow_rays:>12d}", flush=True)
        dev.close()
    if other_tree:
        best_of = {}
        for rep in range(reps):
            for which, tree in (("other", os.path.abspath(other_tree)), ("this", None)):
                env = dict(os.environ)
                env.pop("HRT_ROULETTE_TIME_TREE", None)
                if tree:
                    env["HRT_ROULETTE_TIME_TREE"] = tree
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-rows", "--reps", "2"], env=env, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise SystemExit(f"child ({which}) failed: {r.stderr[-2000:]}")
                for k, (ms, rays) in json.loads(r.stdout.strip().splitlines()[-1]).items():
                    old = best_of.get((k, which), (float("inf"), rays))
                    best_of[(k, which)] = (min(old[0], ms), rays)
        for k in sorted({k for k, _ in best_of}):
            a, b = best_of[(k, "other")], best_of[(k, "this")]
            print(f"without the flag, {k:<28s} other tree {a[0]:7.2f} ms  this tree {b[0]:7.2f} ms  rays {a[1]} / {b[1]}  ({'same' if a[1] == b[1] else 'DIFFERENT'})", flush=True)


def segments():
    from tests.test_gpu_roulette import SEGMENT_CASES, segment_ratio
    d = assets()
    for key, (name, W, H, spp, kw) in SEGMENT_CASES.items():
        hs, dev = scene(d, name)
        cam = hs.camera(W, H)
        rs = [segment_ratio(api, dev, cam, W, H, spp, kw, seed) for seed in range(8)]
        r = np.array([x[0] for x in rs])
        print(f"{key} {W}x{H} {spp}spp {sorted(kw)}: ratio of seed 0 {r[0]:.4f}; seeds 0..7 mean {r.mean():.4f}, std {r.std(ddof=1):.5f}, "
              f"min {r.min():.4f}, max {r.max():.4f}; segments without the flag, seed 0: {rs[0][1]}", flush=True)
        dev.close()


def error():
    d = assets()
    W = H = 128
    hs, dev = scene(d, "cornell_box.yaml")
    cam = hs.camera(W, H)
    ref = np.zeros((H, W, 3))
    for rr in (False, True):
        img, _ = dev.render_tile(cam, api.default_params(W, H, 2048, seed=77777, nee=True, roulette=rr))
        ref += 0.5 * img.astype(np.float64)

    def rms_and_time(spp, rr):
        err, ts = [], []
        for s in range(8):
            p = api.default_params(W, H, spp, seed=500 + s, nee=True, roulette=rr)
            (img, _), t = best(lambda: dev.render_tile(cam, p), 3)
            err.append(np.mean((img.astype(np.float64) - ref) ** 2)); ts.append(t)
        return float(np.sqrt(np.mean(err))), float(np.median(ts)) * 1e3
    spp = 64
    a, ta = rms_and_time(spp, False)
    b, tb = rms_and_time(spp, True)
    spp_eq = max(spp, int(round(spp * ta / tb)))
    c, tc = rms_and_time(spp_eq, True)
    print(f"cornell_box {W}x{H} nee, 8 seeds, RMS against the 2048-spp mean of both estimators:", flush=True)
    print(f"  default  {spp:4d} spp  {ta:7.2f} ms  RMS {a:.5f}", flush=True)
    print(f"  roulette {spp:4d} spp  {tb:7.2f} ms  RMS {b:.5f}   (equal spp: x{b / a:.3f})", flush=True)
    print(f"  roulette {spp_eq:4d} spp  {tc:7.2f} ms  RMS {c:.5f}   (about equal time: x{c / a:.3f})", flush=True)
    dev.close()


def frame(rr, nee):
    d = assets()
    hs, dev = scene(d, "teapot_scene.yaml")
    cam = hs.camera(640, 640)
    p = api.default_params(640, 640, 100, nee=nee, roulette=rr)
    for _ in range(3):
        _, st = dev.render_stripes(cam, p, 8, 0, 1)
    print(f"teapot_scene 640x640 100spp roulette={rr} nee={nee}: rays {st.rays}", flush=True)
    dev.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--other-tree")
    ap.add_argument("--segments", action="store_true")
    ap.add_argument("--error", action="store_true")
    ap.add_argument("--frame", action="store_true")
    ap.add_argument("--roulette", action="store_true")
    ap.add_argument("--nee", action="store_true")
    ap.add_argument("--child-rows", action="store_true")
    a = ap.parse_args()
    if a.child_rows:
        print(json.dumps(rows_without_flag(a.reps)))
    elif a.segments:
        segments()
    elif a.error:
        error()
    elif a.frame:
        frame(a.roulette, a.nee)
    else:
        timing(a.reps, a.other_tree)
