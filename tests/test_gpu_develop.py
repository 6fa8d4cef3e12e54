"""The develop stage (hrt_develop*, include/hrt.h) on the GPU: the kernels of csrc/hrt_develop.hip give the bits of the
numpy restatement of the header's words (tests/develop_np.py) -- film, histogram, metered count and level count to the bit or the
integer, the scale to one fp32 ulp and the metered level to 1e-9, as the header pins them -- on synthetic films of awkward sizes with
every special pixel the definition names, for every level count, strength and exposure mode, and on a real render; the host and
device-pointer forms agree, in place too; the film's render does not notice the stage; and the CLI's flags write what api.develop gives."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import develop_np as dv
from tests.test_develop_cpu import check_lit_square, lit_square

pytestmark = pytest.mark.gpu
F = np.float32
FLOOR = F(2.0 ** -16)

SIZES = [(1, 1), (2, 1), (2, 2), (3, 1),     # no level at all; one level; a row of three: two levels
         (16, 16),                           # one block, 4 levels
         (17, 33), (37, 29),                 # odd sizes at every level, more than one block, 6 levels
         (70, 3), (257, 3)]                  # flat strips: every row clamped above and below; 257 x 3 has all 8 levels
LEVELS = (1, 2, 3, 8)
STRENGTHS = (0.0, 0.05, 1.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _u32(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _same(got, want, what):
    """equal NaN positions, equal bits elsewhere"""
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), (what, "NaN positions", int((nan_g != nan_w).sum()))
    bad = (_bits(got) != _bits(want)) & ~nan_w
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def pixel_with_luminance(target):
    """a valid pixel whose Y, as the header forms it, is exactly the float32 `target` > 0"""
    target = F(target)
    for scale, make in ((F(0.7152), lambda v: (F(0), v, F(0))), (F(0.2126), lambda v: (v, F(0), F(0)))):
        v = F(target / scale)
        for _ in range(8):
            v = np.nextafter(v, F(0))
        for _ in range(17):
            if dv.lum(*make(v)) == target:
                return make(v)
            v = np.nextafter(v, F(np.inf))
    g = F(target / F(0.7152))                                    # most of it from green, the rest -- exact, and tiny -- from red
    for _ in range(4):
        g = np.nextafter(g, F(0))
    rest = F(target - F(0.7152) * g)
    r = F(rest / F(0.2126))
    for _ in range(8):
        r = np.nextafter(r, F(0))
    for _ in range(17):
        if dv.lum(r, g, F(0)) == target:
            return (r, g, F(0))
        r = np.nextafter(r, F(np.inf))
    raise AssertionError(f"no pixel found with luminance {target!r}")


def specials():
    """(pixel, what): the pixels the meter's definition names, each with an exact luminance"""
    out = [(pixel_with_luminance(FLOOR), "at the floor"), (pixel_with_luminance(np.nextafter(FLOOR, F(0))), "below the floor")]
    for e in (-3, 0, 2):
        for k in range(8):
            border = F(2.0 ** e * (1.0 + k / 8.0))
            out.append((pixel_with_luminance(border), "on a bin border"))
            out.append((pixel_with_luminance(np.nextafter(border, F(0))), "an ulp below a bin border"))
    return out


SPECIALS = specials()


def synthetic(W, H, seed):
    """A seeded film [H, W, 3] holding, where it has room for them: runs of exactly equal pixels; zero, -0.0 and negative pixels; NaN,
    +Inf and -Inf pixels alone and in a block; a 1e30 pixel; a luminance at meter_floor and one an ulp below it; luminances exactly on bin
    borders and an ulp below them."""
    r = np.random.default_rng(seed)
    rgb = (r.uniform(0.02, 4.0, (H, W, 1)) * r.uniform(0.5, 1.0, (H, W, 3))).astype(F)
    rgb[r.random((H, W)) < 0.3] = (0.5, 0.25, 0.75)                    # exact ties
    n = W * H
    if n == 1:
        return rgb
    if n < 9:                                                       # 2 x 1, 2 x 2, 3 x 1: an invalid pixel and one at the floor
        rgb[-1, -1] = (0.3, np.nan, 0.2)
        rgb[0, 0] = SPECIALS[0][0]
        return rgb
    flat = rgb.reshape(-1, 3)
    extra = [(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (-0.3, -0.1, -0.2), (0.2, -0.5, 0.1), (np.nan, 0.3, 0.2), (0.1, np.inf, 0.2), (0.1, 0.2, -np.inf),
             (1e30, 2e30, 1e30), (0.0, 1e-6, 0.0)]
    block = np.zeros((H, W), bool)                                  # a block of invalid pixels, wider than the down-sampler's footprint
    block[max(0, H - 6):max(0, H - 6) + 5, W - 9:W - 4] = True
    rgb[block] = np.nan
    spots = r.permutation(np.flatnonzero(~block.ravel()))[:len(SPECIALS) + len(extra)]
    assert len(spots) == len(SPECIALS) + len(extra)
    for i, v in zip(spots, [p for p, _ in SPECIALS] + extra):
        flat[i] = v
    return rgb


def check(api, rgb, what, **kw):
    got, info, hist = api.develop(rgb, return_info=True, return_histogram=True, **kw)
    want, m, winfo, whist = dv.develop(rgb, scale=info.scale, **kw)
    _same(got, want, what)
    invalid = ~np.isfinite(rgb).all(axis=-1)
    assert np.array_equal(_bits(got[invalid]), _bits(rgb[invalid])), (what, "an invalid pixel keeps its bits")
    assert np.array_equal(hist, whist), (what, "histogram", np.flatnonzero(hist != whist)[:8].tolist())
    assert info.metered == winfo["metered"] == int(hist.sum()) and info.levels == winfo["levels"] and info.pad == 0, what
    ulps = abs(_u32(info.scale) - _u32(winfo["scale"]))
    assert ulps <= 1, (what, info.scale, winfo["scale"])
    # float64 rounding over at most 2048 terms of magnitude at most 150: about 3e-11
    assert abs(info.mean_ev - winfo["mean_ev"]) <= 1e-9, (what, info.mean_ev, winfo["mean_ev"])
    return got, info, hist, m


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_kernels_give_the_bits_of_the_restatement(built, size):
    from hobbyraytracer_amd import api
    W, H = size
    rgb = synthetic(W, H, 100 * W + H)
    exists = len(dv.level_sizes(W, H, 8))
    clipped = metered_border = 0
    for levels in LEVELS:
        for s in STRENGTHS:
            for mode, ev in ((dv.NONE, 0.0), (dv.MANUAL, -1.5), (dv.MANUAL, 2.0), (dv.AUTO, 0.0)):
                kw = {"bloom_levels": levels, "bloom_strength": s, "exposure_mode": mode, "exposure_ev": ev}
                got, info, hist, m = check(api, rgb, (size, kw), **kw)
                assert info.levels == min(levels, exists)
                clipped += info.levels < levels
                if mode != dv.AUTO:
                    assert info.scale == (1.0 if mode == dv.NONE else 4.0 if ev == 2.0 else F(2.0 ** -1.5))
                if s == 0.0 and mode != dv.AUTO:                     # no bloom: the film itself, scaled
                    _same(got, dv.develop(rgb, scale=info.scale, exposure_mode=mode, exposure_ev=ev)[0], (size, kw, "s = 0"))
                if mode != dv.AUTO:
                    assert info.metered == 0 and not hist.any() and info.mean_ev == 0.0
                elif s == 0.0 and W * H >= 9:                        # the film's own luminances are metered: the planted ones land where they should
                    metered_border += 1
                    with np.errstate(all="ignore"):
                        l = dv.lum(rgb[..., 0], rgb[..., 1], rgb[..., 2])
                        ok = np.isfinite(rgb).all(axis=-1) & np.isfinite(l)
                    assert info.metered == int((ok & (l >= FLOOR)).sum()) < int(ok.sum())
                    assert hist[_u32(FLOOR) >> 20] >= 1 and hist[(_u32(FLOOR) >> 20) - 1] == 0
    # other keys, windows and clamps; the defaults (no bloom) with the meter alone
    for kw in ({"exposure_mode": dv.AUTO}, {"exposure_mode": dv.AUTO, "bloom_levels": 2, "key": 0.5, "meter_low": 0.0, "meter_high": 1.0},
               {"exposure_mode": dv.AUTO, "bloom_levels": 5, "bloom_strength": 0.3, "meter_low": 0.45, "meter_high": 0.55, "meter_floor": 0.25},
               {"exposure_mode": dv.AUTO, "bloom_levels": 1, "ev_min": 3.0, "ev_max": 3.0}, {"exposure_mode": dv.AUTO, "ev_max": -9.5, "key": 1.0},
               {"exposure_mode": dv.AUTO, "meter_floor": 1e31}):
        check(api, rgb, (size, kw), **kw)
    assert np.array_equal(_bits(api.develop(rgb)), _bits(rgb))                              # the defaults are the identity
    assert api.develop(rgb, exposure_mode=dv.AUTO, meter_floor=1e31, return_info=True)[1].scale == 1.0   # nothing metered
    # the films exercise what they are meant to
    if W * H > 1:
        assert (~np.isfinite(rgb).all(axis=-1)).any()
    if W * H >= 9:
        assert metered_border == len(LEVELS)
    assert (clipped > 0) == (exists < 8), (clipped, exists)
    if W * H < 9:
        assert exists < 3


def test_the_device_form_gives_the_bits_of_the_host_form_on_its_own_stream_in_place_and_without_the_optional_outputs(built):
    import torch
    from hobbyraytracer_amd import api
    W, H = 37, 29
    rgb = synthetic(W, H, 5)
    params = api.develop_defaults(bloom_levels=3, bloom_strength=0.2, exposure_mode=dv.AUTO)
    host, host_info, host_hist = api.develop(rgb, return_info=True, return_histogram=True, bloom_levels=3, bloom_strength=0.2, exposure_mode=dv.AUTO)
    d_rgb = torch.from_numpy(rgb).cuda()
    d_out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    d_info = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    d_hist = torch.full((api.DEVELOP_BINS,), 7, dtype=torch.int32, device="cuda")
    ws = torch.empty(api.develop_workspace_bytes(W, H, 3), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0 and d_info.data_ptr() % 8 == 0

    def info_of(t):
        return api.DevelopInfo.from_buffer_copy(t.cpu().numpy().tobytes())

    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.develop_device(W, H, d_rgb.data_ptr(), d_out.data_ptr(), ws.data_ptr(), d_info.data_ptr(), d_hist.data_ptr(), stream=stream.cuda_stream, params=params)
    stream.synchronize()
    _same(d_out.cpu().numpy(), host, "device form, own stream")
    got = info_of(d_info)
    assert (got.mean_ev, got.scale, got.metered, got.levels, got.pad) == (host_info.mean_ev, host_info.scale, host_info.metered, host_info.levels, 0)
    assert np.array_equal(d_hist.cpu().numpy().view(np.uint32), host_hist)
    assert np.array_equal(_bits(d_rgb.cpu().numpy()), _bits(rgb))                       # the input is only read
    # without the optional outputs, on the null stream: they are left alone; the same workspace again (the call clears its counters)
    d_out.fill_(7.0); d_info.fill_(7); d_hist.fill_(7)
    api.develop_device(W, H, d_rgb.data_ptr(), d_out.data_ptr(), ws.data_ptr(), params=params)
    torch.cuda.synchronize()
    _same(d_out.cpu().numpy(), host, "device form, no info, no histogram")
    assert (d_info == 7).all() and (d_hist == 7).all()
    # in place
    d_both = d_rgb.clone()
    api.develop_device(W, H, d_both.data_ptr(), d_both.data_ptr(), ws.data_ptr(), d_info.data_ptr(), d_hist.data_ptr(), params=params)
    torch.cuda.synchronize()
    _same(d_both.cpu().numpy(), host, "device form, out == rgb")
    assert info_of(d_info).scale == host_info.scale and np.array_equal(d_hist.cpu().numpy().view(np.uint32), host_hist)
    # in place, manual exposure and no bloom: a call that meters nothing still fills the record
    manual = api.develop_defaults(exposure_mode=dv.MANUAL, exposure_ev=1.0)
    d_both = d_rgb.clone()
    api.develop_device(W, H, d_both.data_ptr(), d_both.data_ptr(), ws.data_ptr(), d_info.data_ptr(), d_hist.data_ptr(), params=manual)
    torch.cuda.synchronize()
    _same(d_both.cpu().numpy(), api.develop(rgb, exposure_mode=dv.MANUAL, exposure_ev=1.0), "device form, manual, in place")
    got = info_of(d_info)
    assert (got.mean_ev, got.scale, got.metered, got.levels) == (0.0, 2.0, 0, 0) and not d_hist.any()


@pytest.fixture(scope="module")
def cornell(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "cornell_box.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


def test_a_real_render_with_bloom_and_auto_exposure(cornell):
    api, hs, dev = cornell
    W = H = 64
    film, _ = dev.render_tile(hs.camera(W, H), api.default_params(W, H, 16, seed=3))
    kw = {"bloom_levels": 5, "exposure_mode": dv.AUTO}
    got, info, hist, m = check(api, film, "cornell_box 64 x 64 x 16 spp", **kw)
    assert info.levels == 5 and info.metered > W * H // 2
    print(f"cornell_box 64 x 64 x 16 spp, 5 levels at 0.05, auto: metered {info.metered}, mean_ev {info.mean_ev:.4f}, scale {info.scale:.5g}")


def test_a_lit_square_keeps_its_sum_and_its_reach(built):
    from hobbyraytracer_amd import api
    film = lit_square()
    for s in (1.0, 0.25):
        out, info = api.develop(film, bloom_levels=2, bloom_strength=s, return_info=True)
        assert info.levels == 2
        check_lit_square(film, out, 2)


def test_a_film_rendered_after_a_develop_call_is_the_committed_one(built, tmp_path):
    import importlib.util
    from hobbyraytracer_amd import api
    here = os.path.dirname(__file__)
    spec = importlib.util.spec_from_file_location("make_film_fixtures", os.path.join(here, "golden", "make_film_fixtures.py"))
    mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)
    mk.assets(str(tmp_path))
    want = np.load(os.path.join(here, "golden", "films.npz"))
    scene, W, H, spp = [c for c in mk.CASES if c[0].startswith("cornell_box")][0]
    hs = api.HostScene(os.path.join(here, "golden", "scenes", scene), str(tmp_path))
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        cam = hs.camera(W, H)
        for qn, q in (("ref", api.QUIRKS_REFERENCE), ("fixed", api.QUIRKS_FIXED)):
            api.develop(synthetic(37, 29, 7), bloom_levels=5, exposure_mode=dv.AUTO)
            b = want[f"cornell_box_{qn}"]
            img, st = dev.render_tile(cam, api.default_params(W, H, spp, quirks=q, seed=11))
            same = (img.view(np.uint32) == b.view(np.uint32)) | (np.isnan(img) & np.isnan(b))
            assert same.all(), (qn, int((~same).sum()))
            assert st.rays == int(want[f"cornell_box_{qn}_rays"][0]), qn
    finally:
        dev.close()


def test_cli_develop(cornell, tmp_path, scenes_dir):
    api, hs, dev = cornell
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    W, H, spp = 48, 32, 8
    common = ["s.yaml", "--size", f"{W}x{H}", "--spp", str(spp), "--seed", "2", "--no-progress"]
    keys = ("develop_s", "bloom_levels", "exposure_scale", "exposure_ev")

    def run(*extra):
        r = subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1, r.stdout + r.stderr            # Film::outputFilm's 1 = success (Q-12)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        return json.loads(lines[-1]) if lines else None

    def pfm(name):
        return api.read_pfm(str(tmp_path / name))

    js = run("--bloom", "--exposure", "auto", "--dump-undeveloped", "u.pfm", "--dump-linear", "d.pfm", "--out", "a.png", "--stats")
    plain = run("--dump-linear", "plain.pfm", "--out", "n.png", "--stats")
    assert not any(k in plain for k in keys)                     # none of the flags: none of the keys
    assert (tmp_path / "u.pfm").read_bytes() == (tmp_path / "plain.pfm").read_bytes()
    u, d = pfm("u.pfm"), pfm("d.pfm")
    want, info = api.develop(u, bloom_levels=5, exposure_mode=dv.AUTO, return_info=True)
    _same(d, want, "--bloom --exposure auto")
    assert (_bits(d) != _bits(u)).any()
    assert np.array_equal(api.read_png(str(tmp_path / "a.png")), dev.resolve_u8(d))
    assert all(k in js for k in keys)
    assert js["develop_s"] > 0 and js["bloom_levels"] == info.levels == 5
    assert F(js["exposure_scale"]) == F(info.scale) and js["exposure_ev"] == info.mean_ev
    print(f"cornell_box {W} x {H} x {spp} spp --bloom --exposure auto: scale {info.scale:.5g}, mean_ev {info.mean_ev:.4f}")
    # behind the two cleaning stages: the stage receives that pipeline's film
    run("--despeckle", "--denoise", "--bloom-strength", "0.2", "--bloom-levels", "3", "--exposure-key", "0.3", "--exposure-window", "0.2,0.8",
        "--dump-undeveloped", "u2.pfm", "--dump-linear", "d2.pfm", "--out", "b.png")
    run("--despeckle", "--denoise", "--dump-linear", "clean.pfm", "--out", "c.png")
    assert (tmp_path / "u2.pfm").read_bytes() == (tmp_path / "clean.pfm").read_bytes()
    d2 = pfm("d2.pfm")
    _same(d2, api.develop(pfm("u2.pfm"), bloom_levels=3, bloom_strength=0.2, exposure_mode=dv.AUTO, key=0.3, meter_low=0.2, meter_high=0.8),
          "--despeckle --denoise, then the develop flags")
    assert np.array_equal(api.read_png(str(tmp_path / "b.png")), dev.resolve_u8(d2))
    # manual exposure alone
    js = run("--exposure", "-1.5", "--dump-undeveloped", "u3.pfm", "--dump-linear", "d3.pfm", "--out", "e.png", "--stats")
    assert (tmp_path / "u3.pfm").read_bytes() == (tmp_path / "plain.pfm").read_bytes()
    want, info = api.develop(u, exposure_mode=dv.MANUAL, exposure_ev=-1.5, return_info=True)
    _same(pfm("d3.pfm"), want, "--exposure -1.5")
    assert js["bloom_levels"] == 0 and js["exposure_ev"] == -1.5 and F(js["exposure_scale"]) == F(info.scale) == F(2.0 ** -1.5)
    assert np.array_equal(api.read_png(str(tmp_path / "e.png")), dev.resolve_u8(pfm("d3.pfm")))
