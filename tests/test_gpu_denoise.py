"""The guided denoiser (hrt_denoise*, include/hrt.h) on the GPU: the kernels of csrc/hrt_denoise.hip give the bits of the
numpy restatement of the header's words (tests/denoise_np.py) -- on synthetic films of awkward sizes with every special pixel the
definition names, on a real render with its feature buffers, and with the variance of an adaptive render; in place, out of place, host
and device-pointer forms agree; the film's render does not notice the filter; and the CLI's --denoise writes what api.denoise gives."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import denoise_np as dn

pytestmark = pytest.mark.gpu

SIZES = [(37, 29),   # not a multiple of the 16 x 16 block, smaller than the largest tap reach (32): every iteration skips taps on every side
         (16, 16),   # one block
         (70, 3),    # a flat strip
         (1, 1),     # one pixel
         (2, 2)]     # the smallest film with neighbours


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def synthetic(W, H, seed):
    """A seeded film [H, W, 3], feature buffer [H, W, 8] and variance [H, W] holding, where the film has room for them: a NaN pixel and an
    Inf pixel, misses (alpha 0), fractional alpha, zero normals with a depth (a medium), albedo below the floor, normals of any length."""
    r = np.random.default_rng(seed)
    n = W * H
    y, x = np.mgrid[0:H, 0:W]
    region = ((x * 3) // max(W, 1) + 2 * ((y * 2) // max(H, 1))).ravel()                 # up to six flat regions, so that taps find equals
    albedo = r.uniform(0.05, 0.9, (6, 3)).astype(np.float32)[region] * r.uniform(0.9, 1.1, (n, 3)).astype(np.float32)
    normal = r.normal(size=(6, 3)).astype(np.float32)[region] * r.uniform(0.2, 3.0, (n, 1)).astype(np.float32)
    normal += (0.05 * r.normal(size=(n, 3))).astype(np.float32)
    depth = (r.uniform(2.0, 9.0, 6).astype(np.float32)[region] * r.uniform(0.95, 1.05, n).astype(np.float32))
    alpha = np.ones(n, np.float32)
    rgb = (albedo * r.uniform(0.2, 1.5, (6, 1)).astype(np.float32)[region] + 0.08 * r.standard_normal((n, 3)).astype(np.float32)).astype(np.float32)
    var = r.uniform(0.0, 0.01, n).astype(np.float32)
    pick = r.permutation(n)
    k = max(1, n // 12) if n >= 4 else 0

    def take(i):
        return pick[i * k:(i + 1) * k]
    if k:
        miss = take(0)
        alpha[miss] = 0; depth[miss] = 0; normal[miss] = 0
        albedo[miss] = (0.55, 0.65, 0.8)
        frac = take(1)
        alpha[frac] = r.uniform(0.1, 0.9, frac.size).astype(np.float32)
        depth[frac] *= alpha[frac]; normal[frac] *= alpha[frac][:, None]; albedo[frac] *= alpha[frac][:, None]
        normal[take(2)] = 0                                                                # a medium: no normal, a depth
        albedo[take(3)] = r.uniform(0.0, 0.009, (take(3).size, 3)).astype(np.float32)      # below the floor
        albedo[take(4)[:1]] = 0
        var[take(5)] = 0
        var[take(6)[:1]] = -1.0                                                            # a negative variance counts as 0
    if n >= 12:
        rgb[pick[-1], 1] = np.nan
        rgb[pick[-2]] = (np.inf, 0.5, 0.25)
        rgb[pick[-3], 2] = -np.inf
    aov = np.concatenate([albedo, alpha[:, None], normal, depth[:, None]], axis=1).astype(np.float32)
    return rgb.reshape(H, W, 3), aov.reshape(H, W, 8), var.reshape(H, W)


def _same(got, want, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("with_var", [True, False], ids=["var", "spatial"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_kernels_give_the_bits_of_the_restatement(built, size, with_var):
    from hobbyraytracer_amd import api
    W, H = size
    rgb, aov, var = synthetic(W, H, 100 * W + H)
    var = var if with_var else None
    for iterations in (1, 2, 5, 8):
        for squarings in (0, 7):
            kw = {"iterations": iterations, "normal_squarings": squarings}
            want = dn.denoise(rgb, aov, var, **kw)
            got = api.denoise(rgb, aov, var, **kw)
            _same(got, want, (size, with_var, kw))
    ok = np.isfinite(rgb).all(axis=-1)
    assert np.isfinite(want[ok]).all()                           # (no NaN was produced on the way: the comparison above is of numbers)
    if W * H >= 12:
        assert (~ok).sum() == 3 and np.array_equal(_bits(got[~ok]), _bits(rgb[~ok]))
        assert not np.array_equal(got[ok], rgb[ok])
    # other settings of the remaining parameters
    kw = {"sigma_l": 1.25, "sigma_z": 0.07, "albedo_floor": 0.2}
    _same(api.denoise(rgb, aov, var, **kw), dn.denoise(rgb, aov, var, **kw), (size, with_var, kw))


def test_in_place_and_on_a_stream_of_its_own_the_device_form_gives_the_bits_of_the_host_form(built):
    import torch
    from hobbyraytracer_amd import api
    W, H = 37, 29
    rgb, aov, var = synthetic(W, H, 5)
    host = api.denoise(rgb, aov, var)
    host_spatial = api.denoise(rgb, aov)
    d_rgb, d_aov, d_var = (torch.from_numpy(a).cuda() for a in (rgb, aov, var))
    d_out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(api.denoise_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    assert d_aov.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.denoise_device(W, H, d_rgb.data_ptr(), d_aov.data_ptr(), d_out.data_ptr(), ws.data_ptr(), d_var.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    _same(d_out.cpu().numpy(), host, "device form, out of place, own stream")
    assert np.array_equal(_bits(d_rgb.cpu().numpy()), _bits(rgb))                       # the input is only read
    api.denoise_device(W, H, d_rgb.data_ptr(), d_aov.data_ptr(), d_rgb.data_ptr(), ws.data_ptr(), d_var.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    _same(d_rgb.cpu().numpy(), host, "device form, in place")
    d_rgb2 = torch.from_numpy(rgb).cuda()
    api.denoise_device(W, H, d_rgb2.data_ptr(), d_aov.data_ptr(), d_rgb2.data_ptr(), ws.data_ptr())      # no variance, the null stream
    torch.cuda.synchronize()
    _same(d_rgb2.cpu().numpy(), host_spatial, "device form, in place, spatial variance")
    # the host form in place
    buf = rgb.copy()
    p = api.denoise_defaults()
    import ctypes as C
    fp = C.POINTER(C.c_float)
    api._check(api._hip.hrt_denoise(0, W, H, C.byref(p), buf.ctypes.data_as(fp), aov.ctypes.data_as(fp), None, buf.ctypes.data_as(fp)))
    _same(buf, host_spatial, "host form, in place")


@pytest.fixture(scope="module")
def cornell(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "cornell_box.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


def _raw(aov):
    return np.concatenate([aov["albedo"], aov["alpha"][..., None], aov["normal"], aov["depth"][..., None]], axis=-1)


def test_a_real_render_with_its_feature_buffers_and_the_film_does_not_notice(cornell):
    api, hs, dev = cornell
    W = H = 64
    cam, p = hs.camera(W, H), api.default_params(W, H, 16, seed=3)
    film, _ = dev.render_tile(cam, p)
    aov = dev.render_aov_tile(cam, p)
    got = api.denoise(film, aov)                                  # (the dict of render_aov_tile is accepted as it is)
    _same(got, dn.denoise(film, _raw(aov)), "cornell_box 64 x 64 x 16 spp")
    assert np.isfinite(got).all() and not np.array_equal(got, film)
    again, _ = dev.render_tile(cam, p)                            # a filter call in front of it leaves the film's render alone
    assert np.array_equal(_bits(again), _bits(film))
    # the resolve without a scene gives the scene's bytes
    assert np.array_equal(api.denoise_resolve_u8(got), dev.resolve_u8(got))


def test_the_variance_of_an_adaptive_render(cornell):
    api, hs, dev = cornell
    W = H = 48
    cam, p = hs.camera(W, H), api.default_params(W, H, 32, seed=4)
    ad = api.Adaptive(8, 8, 0.05, 0.01)
    sums = sq = count = None
    for pass_index in range(8):
        sums, sq, count, active, _ = dev.render_stripes_adaptive(cam, p, 8, 0, 1, ad, pass_index, sums, sq, count)
        if active == 0:
            break
    assert count.min() >= 8 and count.max() > count.min()
    film = (sums / count.astype(np.float32)[..., None]).astype(np.float32)
    var = dn.variance_of_mean_luminance(sums, sq, count)
    assert np.isfinite(var).all() and (var > 0).any()
    aov = _raw(dev.render_aov_tile(cam, api.default_params(W, H, 8, seed=4)))
    _same(api.denoise(film, aov, var), dn.denoise(film, aov, var), "adaptive variance")


def test_cli_denoise(cornell, tmp_path, scenes_dir):
    api, hs, dev = cornell
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    W, H = 48, 32
    common = ["s.yaml", "--size", f"{W}x{H}", "--spp", "8", "--seed", "2", "--no-progress"]

    def run(*extra):
        return subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=120)

    r = run("--denoise", "--dump-linear", "filtered.pfm", "--dump-noisy", "noisy.pfm", "--aov", "p", "--aov-spp", "4", "--out", "d.png", "--stats")
    assert r.returncode == 1, r.stdout + r.stderr                # Film::outputFilm's 1 = success (Q-12)
    js = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert js["denoise_s"] > 0 and js["aov_spp"] == 4 and js["samples"] == W * H * 8
    r = run("--dump-linear", "plain.pfm", "--out", "n.png")
    assert r.returncode == 1, r.stderr
    assert (tmp_path / "noisy.pfm").read_bytes() == (tmp_path / "plain.pfm").read_bytes()
    noisy = api.read_pfm(str(tmp_path / "noisy.pfm"))
    part = {n: api.read_pfm(str(tmp_path / f"p.{n}.pfm")) for n in ("albedo", "normal", "depth", "alpha")}
    aov = np.concatenate([part["albedo"], part["alpha"][..., :1], part["normal"], part["depth"][..., :1]], axis=-1)
    want = api.denoise(noisy, aov)
    filtered = api.read_pfm(str(tmp_path / "filtered.pfm"))
    _same(filtered, want, "--dump-linear with --denoise")
    assert not np.array_equal(filtered, noisy)
    assert np.array_equal(api.read_png(str(tmp_path / "d.png")), dev.resolve_u8(filtered))
    assert (tmp_path / "d.png").read_bytes() != (tmp_path / "n.png").read_bytes()
    # the switches: each implies --denoise; the feature files are written only with --aov
    r = run("--denoise-iterations", "2", "--denoise-sigma-l", "1.5", "--denoise-sigma-z", "0.25", "--aov-spp", "4", "--dump-linear", "f2.pfm", "--out", "e.png")
    assert r.returncode == 1, r.stderr
    _same(api.read_pfm(str(tmp_path / "f2.pfm")), api.denoise(noisy, aov, iterations=2, sigma_l=1.5, sigma_z=0.25), "--denoise-* switches")
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pfm")) == ["f2.pfm", "filtered.pfm", "noisy.pfm", "p.albedo.pfm", "p.alpha.pfm", "p.depth.pfm",
                                                                            "p.normal.pfm", "plain.pfm"]
    # usage errors
    for extra in (("--denoise-iterations", "0"), ("--denoise-iterations", "9"), ("--denoise-iterations", "x"), ("--denoise-sigma-l", "0"),
                  ("--denoise-sigma-l", "-1"), ("--denoise-sigma-l", "nan"), ("--denoise-sigma-z", "inf"), ("--denoise-sigma-z", "0"),
                  ("--dump-noisy", "u.pfm"), ("--denoise", "--aov-spp", "9"), ("--denoise", "--aov-spp", "0")):
        r = run("--out", "u.png", *extra)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "u.png").exists() and not (tmp_path / "u.pfm").exists()
