"""The outlier filter (hrt_despeckle*, include/hrt.h) on the GPU: the kernels of csrc/hrt_despeckle.hip give the bits of
the numpy restatement of the header's words (tests/despeckle_np.py), film and map -- on synthetic films of awkward sizes with every
special pixel the definition names, for every window, rank and switch, and on a real render with its measured variance; the host and
device-pointer forms agree; the film's render does not notice the pass; and the CLI's --despeckle writes what api.despeckle gives."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import despeckle_np as ds

pytestmark = pytest.mark.gpu
F = np.float32

SIZES = [(1, 1), (2, 2), (3, 1), (16, 16),   # one pixel; the smallest film with neighbours; a row; one block
         (17, 33), (37, 29),                # windows across block borders and halos, on every side of a block
         (70, 3)]                           # a flat strip: five blocks side by side, every window clipped above and below


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def synthetic(W, H, seed):
    """A seeded film [H, W, 3] and variance [H, W] holding, where the film has room for them: spikes at the corners, on the edges and on
    both sides of the block border at 15 / 16, clusters of two and three spikes, runs of exactly equal pixels, zero and negative pixels (a
    positive pixel among negative ones too), NaN / +Inf / -Inf pixels alone, beside a spike and filling a whole 5 x 5 window, and
    variances that open the gate, close it, and are zero, negative and NaN."""
    r = np.random.default_rng(seed)
    rgb = (r.uniform(0.2, 1.2, (H, W, 1)) * r.uniform(0.5, 1.0, (H, W, 3))).astype(F)
    tie = r.random((H, W)) < 0.3
    rgb[tie] = (0.5, 0.25, 0.75)                                      # exact ties, among them the largest neighbours of many pixels

    def put(x, y, value):
        if 0 <= x < W and 0 <= y < H:
            rgb[y, x] = value
            return True
        return False

    def spike(x, y, k):
        if 0 <= x < W and 0 <= y < H:
            rgb[y, x] = rgb[y, x] * F(k)
    if W * H == 1:
        return rgb, np.full((H, W), 0.01, F)
    for n, (x, y) in enumerate([(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (0, H // 2), (W - 1, H // 2), (W // 2, H - 1),
                                (15, 5), (16, 9), (5, 15), (9, 16), (15, 15), (16, 16), (15, 1), (16, 1),
                                (8, 20), (9, 20), (8, 21), (25, 2), (26, 2), (27, 1)]):
        spike(x, y, 20 + 7 * n)
    if W * H >= 9:
        put(3, 1, (0.0, 0.0, 0.0))
        put(5, 2, (0.0, 0.0, 0.0))
        put(6, 1, (-0.3, -0.1, -0.2))
        for y in range(9, 12):                                        # a positive pixel whose whole 3 x 3 neighbourhood is negative
            for x in range(1, 4):
                put(x, y, (-0.2, -0.3, -0.1))
        put(2, 10, (3.0, 2.0, 1.0))
        put(4, 0, (np.nan, 0.3, 0.2))                                 # alone
        put(W // 2 + 1, 0, (0.1, np.inf, 0.2))                        # beside the spike at (W // 2, 0)
        put(1, H - 1, (0.1, 0.2, -np.inf))                            # beside the corner spike
        put(12, 2, (1e30, 2e30, 1e30))                                # a huge finite pixel: its shares swamp its neighbours
    if W >= 12 and H >= 3:                                            # a whole 5 x 5 window (clipped to the film) of invalid pixels
        x0, y0 = W - 9, max(0, H - 9)
        rgb[y0:y0 + 5, x0:x0 + 5] = np.nan
        spike(x0 - 1, y0 + 1, 40)                                     # ... with a spike on its rim
    if W * H < 9:                                                     # 2 x 2 and 3 x 1: a spike and an invalid pixel
        rgb[-1, -1] = np.nan
    with np.errstate(all="ignore"):
        l = ds.lum(rgb[..., 0], rgb[..., 1], rgb[..., 2])
        var = np.square(np.nan_to_num(l, posinf=1.0, neginf=1.0) * r.uniform(0.0, 1.0, (H, W))).astype(F)
    pick = r.random((H, W))
    var[pick < 0.10] = 0.0
    var[(pick >= 0.10) & (pick < 0.15)] = -1.0
    var[(pick >= 0.15) & (pick < 0.20)] = np.nan
    return rgb, var


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_kernels_give_the_bits_of_the_restatement(built, size):
    from hobbyraytracer_amd import api
    W, H = size
    rgb, var = synthetic(W, H, 100 * W + H)
    outliers = repaired = gated = 0
    for radius in (1, 2):
        for rank in (1, 2, 3, 4):
            for ratio in (1.5, 4.0):
                for repair in (1, 0):
                    kw = {"radius": radius, "rank": rank, "ratio": ratio, "repair_invalid": repair}
                    free = None
                    for v in (None, var):
                        want, want_map = ds.despeckle(rgb, v, **kw)
                        got, got_map = api.despeckle(rgb, v, return_map=True, **kw)
                        _same(got, want, (size, v is not None, kw))
                        _same(got_map, want_map, (size, v is not None, kw, "map"))
                        outliers += int((got_map > 0).sum())
                        repaired += int((got_map == -1).sum())
                        if v is None:
                            free = got_map
                        else:
                            gated += int(((free > 0) & (got_map == 0)).sum())
    kw = {"gate_z": 0.0, "radius": 2}
    _same(api.despeckle(rgb, var, **kw), ds.despeckle(rgb, None, **kw)[0], (size, "gate_z 0 is no gate"))
    kw = {"gate_z": 0.5}
    got, got_map = api.despeckle(rgb, var, return_map=True, **kw)
    want, want_map = ds.despeckle(rgb, var, **kw)
    _same(got, want, (size, kw))
    _same(got_map, want_map, (size, kw, "map"))
    assert np.array_equal(_bits(api.despeckle(rgb)), _bits(ds.despeckle(rgb)[0]))          # without the map
    if W * H >= 9:                                               # the films exercise what they are meant to
        assert outliers > 0 and repaired > 0 and gated > 0, (outliers, repaired, gated)
    if W >= 12:                                                  # the centre of the invalid block keeps its bits, even when repairing
        x0, y0 = W - 9, max(0, H - 9)
        cy = min(y0 + 2, H - 1)
        got, got_map = api.despeckle(rgb, radius=2, return_map=True)
        assert np.array_equal(_bits(got[cy, x0 + 2]), _bits(rgb[cy, x0 + 2])) and got_map[cy, x0 + 2] == 0
        assert got_map[cy, x0] == -1                             # ... while the block's rim is repaired


def test_on_a_stream_of_its_own_the_device_form_gives_the_bits_of_the_host_form(built):
    import torch
    from hobbyraytracer_amd import api
    W, H = 37, 29
    rgb, var = synthetic(W, H, 5)
    host, host_map = api.despeckle(rgb, var, return_map=True, radius=2, rank=3)
    host_free = api.despeckle(rgb)
    d_rgb, d_var = torch.from_numpy(rgb).cuda(), torch.from_numpy(var).cuda()
    d_out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    d_map = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(api.despeckle_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.despeckle_device(W, H, d_rgb.data_ptr(), d_out.data_ptr(), ws.data_ptr(), d_var.data_ptr(), d_map.data_ptr(), stream=stream.cuda_stream,
                         params=api.despeckle_defaults(radius=2, rank=3))
    stream.synchronize()
    _same(d_out.cpu().numpy(), host, "device form, own stream")
    _same(d_map.cpu().numpy(), host_map, "device form, own stream, map")
    assert np.array_equal(_bits(d_rgb.cpu().numpy()), _bits(rgb))                       # the input is only read
    api.despeckle_device(W, H, d_rgb.data_ptr(), d_out.data_ptr(), ws.data_ptr())      # no variance, no map, the null stream
    torch.cuda.synchronize()
    _same(d_out.cpu().numpy(), host_free, "device form, no variance")
    _same(d_map.cpu().numpy(), host_map, "the map is left alone when none is asked for")
    with pytest.raises(api.HrtError):
        api.despeckle_device(W, H, d_rgb.data_ptr(), d_rgb.data_ptr(), ws.data_ptr())


@pytest.fixture(scope="module")
def cornell(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "cornell_box.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


def test_a_real_render_under_roulette_with_its_measured_variance(cornell):
    api, hs, dev = cornell
    W = H = 64
    cam, p = hs.camera(W, H), api.default_params(W, H, 16, seed=3, roulette=True)
    film, var = dev.render_stripes_with_variance(cam, p, batches=4)
    assert np.isfinite(var).all() and (var > 0).any()
    for v in (var, None):
        got, got_map = api.despeckle(film, v, return_map=True)
        want, want_map = ds.despeckle(film, v)
        _same(got, want, ("cornell_box 64 x 64 x 16 spp, roulette", v is not None))
        _same(got_map, want_map, ("its map", v is not None))
        assert (got_map > 0).any()
        print(f"cornell_box 64 x 64 x 16 spp, roulette, variance {'given' if v is not None else 'absent'}: {int((got_map > 0).sum())} outliers")
        for k in range(3):                                       # no energy left the film
            a, b = film[..., k].astype(np.float64).sum(), got[..., k].astype(np.float64).sum()
            assert abs(a - b) <= 1e-5 * a


def test_a_film_rendered_after_a_despeckle_call_is_the_committed_one(built, tmp_path):
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
            rgb, var = synthetic(37, 29, 7)
            api.despeckle(rgb, var)
            b = want[f"cornell_box_{qn}"]
            img, st = dev.render_tile(cam, api.default_params(W, H, spp, quirks=q, seed=11))
            same = (img.view(np.uint32) == b.view(np.uint32)) | (np.isnan(img) & np.isnan(b))
            assert same.all(), (qn, int((~same).sum()))
            assert st.rays == int(want[f"cornell_box_{qn}_rays"][0]), qn
    finally:
        dev.close()


def test_cli_despeckle(cornell, tmp_path, scenes_dir):
    api, hs, dev = cornell
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    W, H, spp = 48, 32, 8
    common = ["s.yaml", "--size", f"{W}x{H}", "--spp", str(spp), "--seed", "2", "--no-progress"]

    def run(*extra):
        return subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=120)

    def pfm(name):
        return api.read_pfm(str(tmp_path / name))

    # the stage alone: no variance, so the gate is off and the program says so
    r = run("--despeckle", "--despeckle-map", "map.pfm", "--dump-noisy", "noisy.pfm", "--dump-linear", "clean.pfm", "--out", "d.png", "--stats")
    assert r.returncode == 1, r.stdout + r.stderr                # Film::outputFilm's 1 = success (Q-12)
    assert r.stderr.count("the variance gate is off") == 1
    r2 = run("--dump-linear", "plain.pfm", "--out", "n.png")
    assert r2.returncode == 1, r2.stderr
    assert (tmp_path / "noisy.pfm").read_bytes() == (tmp_path / "plain.pfm").read_bytes()
    noisy, clean, dmap = pfm("noisy.pfm"), pfm("clean.pfm"), pfm("map.pfm")
    want, want_map = api.despeckle(noisy, return_map=True)
    _same(clean, want, "--dump-linear with --despeckle")
    for k in range(3):
        _same(dmap[..., k], want_map, "--despeckle-map")
    js = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert js["despeckle_s"] > 0 and js["despeckle_pixels"] == int((want_map > 0).sum()) > 0 and js["despeckle_repaired"] == int((want_map < 0).sum())
    assert "denoise_s" not in js
    assert np.array_equal(api.read_png(str(tmp_path / "d.png")), dev.resolve_u8(clean))
    # the two dumps differ exactly where the map is non-zero or a window holds a non-zero map
    touched = np.zeros((H, W), bool)
    for y, x in np.argwhere(want_map > 0):                       # an outlier moves itself and deals a share to its window's valid pixels
        touched[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
    touched = (touched & np.isfinite(noisy).all(axis=-1)) | (want_map != 0)
    assert np.array_equal((_bits(noisy) != _bits(clean)).any(axis=-1), touched)
    # ahead of the denoiser, with the measured variance: both stages get it, the denoiser unchanged; the switches imply --despeckle
    r = run("--despeckle-ratio", "1.5", "--despeckle-rank", "3", "--despeckle-radius", "2", "--despeckle-gate", "3", "--denoise-variance", "measured",
            "--dump-variance", "var.pfm", "--despeckle-map", "map2.pfm", "--dump-noisy", "noisy2.pfm", "--dump-linear", "both.pfm", "--aov", "p",
            "--aov-spp", "4", "--out", "e.png", "--stats")
    assert r.returncode == 1, r.stdout + r.stderr
    assert "the variance gate is off" not in r.stderr
    assert (tmp_path / "noisy2.pfm").read_bytes() == (tmp_path / "plain.pfm").read_bytes()
    var = pfm("var.pfm")[..., 0]
    part = {n: pfm(f"p.{n}.pfm") for n in ("albedo", "normal", "depth", "alpha")}
    aov = np.concatenate([part["albedo"], part["alpha"][..., :1], part["normal"], part["depth"][..., :1]], axis=-1)
    mid, mid_map = api.despeckle(noisy, var, return_map=True, ratio=1.5, rank=3, radius=2, gate_z=3.0)
    _same(pfm("map2.pfm")[..., 0], mid_map, "--despeckle-map under --denoise")
    both = pfm("both.pfm")
    _same(both, api.denoise(mid, aov, var, sigma_l=6.0), "--despeckle, then --denoise")
    assert np.array_equal(api.read_png(str(tmp_path / "e.png")), dev.resolve_u8(both))
    js = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert js["despeckle_s"] > 0 and js["denoise_s"] > 0 and js["despeckle_pixels"] == int((mid_map > 0).sum())
    # --adaptive: the stage alone is given the variance of the adaptive buffers
    r = run("--adaptive", "0.05", "--min-samples", "4", "--progressive", "2", "--despeckle", "--despeckle-map", "map3.pfm", "--dump-noisy", "na.pfm",
            "--dump-linear", "fa.pfm", "--out", "a.png")
    assert r.returncode == 1, r.stdout + r.stderr
    assert "the variance gate is off" not in r.stderr
    ad = api.Adaptive(4, 2, 0.05, 0.01)
    sums = sq = count = None
    for pass_index in range(8):
        sums, sq, count, active, _ = dev.render_stripes_adaptive(hs.camera(W, H), api.default_params(W, H, spp, seed=2), 8, 0, 1, ad, pass_index, sums, sq, count)
        if active == 0:
            break
    got, got_map = api.despeckle(pfm("na.pfm"), api.adaptive_variance(sums, sq, count), return_map=True)
    _same(pfm("fa.pfm"), got, "--adaptive --despeckle")
    _same(pfm("map3.pfm")[..., 0], got_map, "--adaptive --despeckle-map")
