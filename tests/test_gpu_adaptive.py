"""Adaptive sampling (include/hrt.h hrt_render_stripes_adaptive*): per-pixel sample counts driven by the noise of the mean
luminance.  Every path is keyed by (pixel, sample, bounce), so a pixel that took n samples holds exactly the fp32 sum of the
first n samples of the uniform render -- the tests pin the new path bit for bit to hrt_render_stripes /
hrt_render_stripes_accumulate, which the oracle tests pin in turn."""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _luma(rgb):
    """Y of hrt.h in float32, three products added left to right (the library builds with -ffp-contract=off)."""
    rgb = rgb.astype(np.float32)
    return np.float32(0.2126) * rgb[..., 0] + np.float32(0.7152) * rgb[..., 1] + np.float32(0.0722) * rgb[..., 2]


def _rule(sums, sq, n, thr, floor):
    """The stopping rule restated in float64 -> (lhs, rhs, slack): the pixel stops when lhs < rhs.  slack bounds the fp32
    rounding of sq - n*m*m (cancellation) that the float64 restatement cannot see."""
    n = np.asarray(n, np.float64)
    m = _luma(sums).astype(np.float64) / n
    sq = sq.astype(np.float64)
    var = np.maximum(0.0, (sq - n * m * m) / (n - 1.0))
    lhs = var / n
    rhs = (thr * np.maximum(m, floor)) ** 2
    slack = 1e-3 * np.maximum(lhs, rhs) + 8 * np.finfo(np.float32).eps * (np.abs(sq) + n * m * m) / ((n - 1.0) * n)
    return lhs, rhs, slack


def _run(dev, cam, p, ad, R=8, rank=0, G=1):
    """All passes -> (sums, sq, count, passes, samples counted)."""
    sums = sq = count = None
    k, samples = 0, 0
    while True:
        sums, sq, count, active, st = dev.render_stripes_adaptive(cam, p, R, rank, G, ad, k, sums, sq, count)
        samples += st.samples
        if active == 0:
            return sums, sq, count, k, samples
        k += 1


@pytest.fixture(scope="module")
def cornell(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(f"{scenes_dir}/cornell_box.yaml", assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    W = H = 64
    spp = 64
    cam = hs.camera(W, H)
    # per-sample radiance and the undivided running sums of the uniform render: params.samples = spp + 1 keeps
    # hrt_render_stripes_accumulate from dividing (the kernels key paths by (pixel, sample, bounce) and never read it)
    pu = api.default_params(W, H, spp + 1)
    rad = np.empty((spp, H, W, 3), np.float32)
    for s in range(spp):
        acc = np.zeros((H, W, 3), np.float32)
        dev.render_stripes_accumulate(cam, pu, 8, 0, 1, acc, s, 1)
        rad[s] = acc
    prefix = np.empty((spp + 1, H, W, 3), np.float32)
    prefix[0] = 0
    acc = np.zeros((H, W, 3), np.float32)
    for s in range(0, spp, 8):
        dev.render_stripes_accumulate(cam, pu, 8, 0, 1, acc, s, 8)
        prefix[s + 8] = acc
    yield dict(api=api, hs=hs, dev=dev, cam=cam, W=W, H=H, spp=spp, rad=rad, prefix=prefix)
    dev.close()


def test_threshold_zero_is_the_uniform_render(built, assets, scenes_dir):
    """threshold 0 never stops a pixel early: every count ends at `samples` and the mean is bit for bit render_stripes,
    for 1, 2 and 3 stripe partitions; the device mean kernel gives the same bits."""
    from hobbyraytracer_amd import api
    hs = api.HostScene(f"{scenes_dir}/material_zoo.yaml", assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    W, H, spp, R = 72, 56, 16, 8
    cam, p = hs.camera(W, H), api.default_params(W, H, spp)
    ad = api.Adaptive(4, 5, 0.0, 0.0)
    for G in (1, 2, 3):
        for rank in range(G):
            ref, _ = dev.render_stripes(cam, p, R, rank, G)
            sums, sq, count, passes, samples = _run(dev, cam, p, ad, R, rank, G)
            assert passes == 4, (G, rank, passes)               # 4, then 5 + 5 + 2
            assert (count == spp).all(), (G, rank)
            assert samples == count.sum()
            mean = sums / count.astype(np.float32)[..., None]
            assert np.array_equal(mean.view(np.uint32), ref.view(np.uint32)), (G, rank)
    mean, count, st = dev.render_adaptive(cam, p, ad)
    ref, _ = dev.render_stripes(cam, p, R, 0, 1)
    assert np.array_equal(mean.view(np.uint32), ref.view(np.uint32)) and st.samples == W * H * spp
    dev.close()


def test_device_form_and_mean_kernel(built, assets, scenes_dir):
    """hrt_render_stripes_adaptive_device on torch buffers + hrt_adaptive_mean_device == the host form, bit for bit."""
    import torch
    from hobbyraytracer_amd import api
    hs = api.HostScene(f"{scenes_dir}/cornell_box.yaml", assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    W, H, spp = 48, 40, 24
    cam, p = hs.camera(W, H), api.default_params(W, H, spp)
    ad = api.Adaptive(4, 4, 0.05, 0.01)
    sums_h, sq_h, count_h, _, _ = _run(dev, cam, p, ad)
    stream = torch.cuda.Stream()
    sums = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
    sq = torch.full((H, W), float("nan"), dtype=torch.float32, device="cuda")
    count = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
    mean = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    k = 0
    with torch.cuda.stream(stream):
        while dev.render_stripes_adaptive_device(cam, p, 8, 0, 1, ad, sums.data_ptr(), sq.data_ptr(), count.data_ptr(), k, stream.cuda_stream):
            k += 1
        dev.adaptive_mean_device(sums.data_ptr(), count.data_ptr(), W * H, mean.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(sums.cpu().numpy().view(np.uint32), sums_h.view(np.uint32))
    assert np.array_equal(sq.cpu().numpy().view(np.uint32), sq_h.view(np.uint32))
    assert np.array_equal(count.cpu().numpy(), count_h)
    ref = sums_h / count_h.astype(np.float32)[..., None]
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    dev.stats()
    dev.close()


def _threshold_with_both_kinds(c, ad_of):
    """The first of a few thresholds at which the cornell render has stopped pixels AND pixels that ran to the end."""
    p = c["api"].default_params(c["W"], c["H"], c["spp"])
    for thr in (0.02, 0.04, 0.08, 0.15, 0.3):
        out = _run(c["dev"], c["cam"], p, ad_of(thr))
        count = out[2]
        if (count < c["spp"]).any() and (count == c["spp"]).any():
            return thr, out
    pytest.fail("no threshold gave both stopped and unstopped pixels")


def test_prefix_property_sq_and_stopping_decisions(cornell):
    """With a real threshold: sums of a pixel that took n samples == the uniform accumulation after samples [0, n), bit for
    bit; sq == the float32 sum, in sample order, of each sample's Y*Y; every pixel that stopped early satisfies the rule
    at n, and every pixel past min_samples failed it at n - pass_samples (pixels within rounding of the boundary skipped)."""
    c = cornell
    api, spp = c["api"], c["spp"]
    mn, ps, floor = 8, 8, 0.01
    thr, (sums, sq, count, passes, samples) = _threshold_with_both_kinds(c, lambda t: api.Adaptive(mn, ps, t, floor))
    assert set(np.unique(count)) <= set(range(mn, spp + 1, ps))
    assert samples == count.sum()
    rad, prefix = c["rad"], c["prefix"]
    yy = _luma(rad) * _luma(rad)
    sq_prefix = np.zeros((spp + 1,) + yy.shape[1:], np.float32)
    for s in range(spp):
        sq_prefix[s + 1] = sq_prefix[s] + yy[s]
    iy, ix = np.indices(count.shape)
    assert np.array_equal(sums.view(np.uint32), prefix[count, iy, ix].view(np.uint32))
    assert np.array_equal(sq.view(np.uint32), sq_prefix[count, iy, ix].view(np.uint32))
    # the decision that ended each pixel
    stopped = count < spp
    lhs, rhs, slack = _rule(sums, sq, count, thr, floor)
    clear = np.abs(lhs - rhs) > slack
    assert (lhs[stopped & clear] < rhs[stopped & clear]).all()
    # ... and the one before it kept the pixel going
    went_on = count > mn
    prev = np.maximum(count - ps, mn)
    lhs, rhs, slack = _rule(prefix[prev, iy, ix], sq_prefix[prev, iy, ix], prev, thr, floor)
    clear = np.abs(lhs - rhs) > slack
    assert not (lhs[went_on & clear] < rhs[went_on & clear]).any()
    assert (stopped & clear).sum() > 0 and (went_on & clear).sum() > 0
    print(f"cornell 64x64x{spp}, threshold {thr}: {passes} passes, {samples} samples = {samples / count.size / spp:.3f} of uniform")


def test_inputs_and_refusals(cornell):
    """Pass 0 reads none of the buffers; invalid schedules and the megakernel are refused; a finished render answers 0."""
    c = cornell
    api, dev, cam, W, H = c["api"], c["dev"], c["cam"], c["W"], c["H"]
    p = api.default_params(W, H, 16)
    ad = api.Adaptive(4, 4, 0.1, 0.01)
    a = dev.render_stripes_adaptive(cam, p, 8, 0, 1, ad, 0, np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32),
                                    np.zeros((H, W), np.int32))
    b = dev.render_stripes_adaptive(cam, p, 8, 0, 1, ad, 0, np.full((H, W, 3), np.nan, np.float32), np.full((H, W), np.nan, np.float32),
                                    np.full((H, W), 12345, np.int32))
    assert a[3] == b[3] == W * H and a[4].samples == W * H * 4
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # a NaN in sq keeps the pixel active to the end
    sums, sq, count = b[0], b[1].copy(), b[2]
    sq[3, 5] = np.nan
    k = 1
    while True:
        sums, sq, count, active, _ = dev.render_stripes_adaptive(cam, p, 8, 0, 1, ad, k, sums, sq, count)
        if not active:
            break
        k += 1
    assert count[3, 5] == 16
    with pytest.raises(api.HrtError) as e:
        dev.render_stripes_adaptive(cam, api.default_params(W, H, 16, megakernel=True), 8, 0, 1, ad, 0)
    assert e.value.status == api.HRT_ERR_UNSUPPORTED
    for bad in ((1, 4, 0.1, 0.0), (17, 4, 0.1, 0.0), (4, 0, 0.1, 0.0), (4, 4, -0.1, 0.0), (4, 4, float("nan"), 0.0),
                (4, 4, 0.1, -1.0), (4, 4, 0.1, float("nan"))):
        with pytest.raises(api.HrtError) as e:
            dev.render_stripes_adaptive(cam, p, 8, 0, 1, api.Adaptive(*bad), 0)
        assert e.value.status == api.HRT_ERR_INVALID, bad
    with pytest.raises(api.HrtError) as e:
        dev.render_stripes_adaptive(cam, p, 8, 0, 1, ad, -1)
    assert e.value.status == api.HRT_ERR_INVALID
    # pass 4 of a 4 + 4k schedule at 16 spp: every pixel is at 16 -> nothing left to do, buffers untouched
    s0 = np.full((H, W, 3), 2.0, np.float32)
    out = dev.render_stripes_adaptive(cam, p, 8, 0, 1, ad, 4, s0.copy(), np.zeros((H, W), np.float32), np.full((H, W), 16, np.int32))
    assert out[3] == 0 and out[4].samples == 0 and np.array_equal(out[0], s0)


def test_headline_scene_takes_fewer_samples(built, assets, scenes_dir):
    """teapot_scene.yaml at 640x640, 100 spp: a moderate threshold takes fewer samples than the uniform render."""
    from hobbyraytracer_amd import api
    hs = api.HostScene(f"{scenes_dir}/teapot_scene.yaml", assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    W = H = 640
    spp = 100
    cam, p = hs.camera(W, H), api.default_params(W, H, spp)
    dev.render_stripes(cam, p, 8, 0, 1)                                  # warm-up (workspace, code objects)
    t0 = time.perf_counter()
    ref, _ = dev.render_stripes(cam, p, 8, 0, 1)
    t_uniform = time.perf_counter() - t0
    t0 = time.perf_counter()
    mean, count, st = dev.render_adaptive(cam, p, api.Adaptive(16, 16, 0.05, 0.01))
    t_adaptive = time.perf_counter() - t0
    frac = count.sum() / (W * H * spp)
    rms = float(np.sqrt(np.mean((mean.astype(np.float64) - ref) ** 2)))
    print(f"teapot 640x640x{spp}: adaptive 0.05 takes {count.sum()} samples ({frac:.3f} of uniform) in {t_adaptive * 1e3:.1f} ms "
          f"(uniform {t_uniform * 1e3:.1f} ms), RMS vs the uniform render {rms:.4g}")
    assert st.samples == count.sum()
    assert count.min() >= 16 and count.max() <= spp
    assert frac < 1.0
    dev.close()


def test_cli_adaptive_sample_map(built, assets, scenes_dir, tmp_path):
    """--adaptive T --min-samples N --progressive N --sample-map: the PFM holds the API's counts, --dump-linear its mean, the PNG
    its tonemapped mean; --stats reports the samples taken."""
    import json
    import shutil
    import subprocess
    from hobbyraytracer_amd import api
    shutil.copy(os.path.join(scenes_dir, "cornell_box.yaml"), tmp_path / "c.yaml")
    W, H, spp = 40, 32, 24
    cmd = [api.CLI_PATH, "c.yaml", "--size", f"{W}x{H}", "--spp", str(spp), "--adaptive", "0.05", "--min-samples", "8", "--progressive", "4",
           "--sample-map", "map.pfm", "--dump-linear", "lin.pfm", "--out", "o.png", "--stats", "--assets", assets]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    js = json.loads(line)
    hs = api.HostScene(str(tmp_path / "c.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    mean, count, st = dev.render_adaptive(hs.camera(W, H), api.default_params(W, H, spp), api.Adaptive(8, 4, 0.05, 0.01))
    smap = api.read_pfm(str(tmp_path / "map.pfm"))
    assert smap.shape == (H, W, 3) and (smap == count[..., None].astype(np.float32)).all()
    assert np.array_equal(api.read_pfm(str(tmp_path / "lin.pfm")).view(np.uint32), mean.view(np.uint32))
    assert np.array_equal(api.read_png(str(tmp_path / "o.png")), dev.resolve_u8(mean))
    assert js["samples_taken"] == js["samples"] == int(count.sum())
    assert abs(js["sample_fraction"] - count.sum() / (W * H * spp)) < 1e-5
    dev.close()
