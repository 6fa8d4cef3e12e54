"""The measured variance (hrt_variance_*, hrt_adaptive_variance*, include/hrt.h) on the GPU: the kernels of
csrc/hrt_variance.hip give the bits of the numpy restatement of the header's words (tests/variance_np.py) -- on synthetic buffers of
awkward sizes with every special value, for every batching, on real renders taken in passes and on an adaptive render; host and
device-pointer forms agree; the film does not depend on the batching or notice the calls; and the CLI's --denoise-variance measured writes
what the Python pipeline gives."""
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

from tests import denoise_np as dn
from tests import variance_np as vn

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(1,), (255,), (256,), (257,), (29, 37)]            # one pixel; one block less one, exactly, plus one; a film of odd sizes (5 blocks)
BATCHINGS = [(4, 4), (3, 3, 2), (2, 1, 5), (1, 1, 1, 1, 4), (5, 3)]     # 2, 3 and 5 batches, equal and unequal, a shorter last one


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def _same_state(got, want, what):
    """Bit for bit, except that a NaN is a NaN: IEEE 754 leaves the sign and payload of a NaN an operation produces to the
    implementation, and the variance -- the output -- never holds one (max(0, NaN) is 0)."""
    bad = (_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def synthetic_sums(shape, counts, seed, special=True):
    """Seeded accumulation buffers after each batch, [(*shape, 3)] per batch: running fp32 sums of positive samples; with `special`, where
    there is room, pixels that are zero throughout, negative, NaN from some batch on, +Inf and -Inf from some batch on."""
    r = np.random.default_rng(seed)
    n = int(np.prod(shape))
    level = r.uniform(0.05, 3.0, (n, 3))
    sums, after = np.zeros((n, 3), F), []
    for j, c in enumerate(counts):
        for _ in range(c):
            sums = sums + np.abs(level * (1.0 + 0.5 * r.standard_normal((n, 3)))).astype(F)
        buf = sums.copy()
        if special and n >= 16:
            buf[3] = 0.0
            buf[4] = -buf[4]
            if j >= 1:
                buf[5, 1] = np.nan
                buf[6] = (np.inf, 1.0, 2.0)
            if j >= len(counts) - 1:
                buf[7, 2] = -np.inf
            buf[8] = (0.0, -0.0, 0.0)
        after.append(buf.reshape(*shape, 3))
    return after


def gpu_from_batches(api, buffers, counts, samples=None):
    """vn.from_batches on the GPU through the host forms; every intermediate state is compared too"""
    done, state, want = 0, None, None
    for j, (buf, c) in enumerate(zip(buffers, counts)):
        scale = float(samples) if (samples is not None and j == len(counts) - 1) else 1.0
        state_in, before = state, (None if state is None else state.copy())
        state = api.variance_fold(buf, done, c, state_in, scale=scale)
        want = vn.fold(buf, scale, done, c, want)
        _same_state(state, want, ("state after batch", j))
        if before is not None:
            assert np.array_equal(_bits(before), _bits(state_in))        # the caller's state is not written: a new array comes back
        state = np.where(np.isnan(state), want, state).astype(F)          # carry the restatement's NaN bits, so that only numbers differ
        done += c
    return api.variance_finish(state, done, len(counts)), vn.finish(want, done, len(counts))


@pytest.mark.parametrize("shape", SIZES, ids=["x".join(map(str, s)) for s in SIZES])
def test_fold_and_finish_give_the_bits_of_the_restatement(built, shape):
    from hobbyraytracer_amd import api
    for k, counts in enumerate(BATCHINGS):
        after = synthetic_sums(shape, counts, 1000 * k + int(np.prod(shape)))
        total = sum(counts)
        got, want = gpu_from_batches(api, after, counts)                  # scale 1 throughout: undivided sums
        _same(got, want, (shape, counts, "sums"))
        assert got.shape == tuple(shape) and not np.isnan(got).any()
        if np.prod(shape) >= 16:
            flat = got.reshape(-1)
            assert flat[3] == 0 and flat[5] == 0 and flat[8] == 0 and (flat[9:] > 0).all() and flat[4] > 0
        divided = after[:-1] + [(after[-1] / F(total)).astype(F)]         # the buffer whose last pass has divided
        got, want = gpu_from_batches(api, divided, counts, samples=total)
        _same(got, want, (shape, counts, "divided"))


@pytest.mark.parametrize("shape", SIZES, ids=["x".join(map(str, s)) for s in SIZES])
def test_the_adaptive_variance_gives_the_bits_of_the_restatement(built, shape):
    from hobbyraytracer_amd import api
    r = np.random.default_rng(int(np.prod(shape)))
    n = int(np.prod(shape))
    count = r.integers(0, 40, n).astype(np.int32)
    count[:min(n, 6)] = [0, 1, 2, 3, 1, 0][:min(n, 6)]
    y = r.uniform(0.05, 2.0, n)
    sums = (np.stack([y, y * 0.8, y * 1.3], axis=-1) * count[:, None]).astype(F)
    m = dn.lum(sums[:, 0], sums[:, 1], sums[:, 2]) / np.maximum(count, 1).astype(F)
    sq = (count * m * m * r.uniform(0.9, 1.6, n)).astype(F)              # below n m m for some: the clamp
    if n >= 16:
        sums[9, 0] = np.nan; sums[10] = np.inf; sq[11] = np.inf; sq[12] = -np.inf; sums[13] = -sums[13]; sums[14] = 0; sq[14] = 0
    sums, sq, count = sums.reshape(*shape, 3), sq.reshape(shape), count.reshape(shape)
    got = api.adaptive_variance(sums, sq, count)
    _same(got, vn.adaptive(sums, sq, count), shape)
    ok = count >= 2
    _same(got[ok], dn.variance_of_mean_luminance(sums, sq, count)[ok], "variance_of_mean_luminance where count >= 2")
    assert (got[~ok] == 0).all() and not np.isnan(got).any()


def test_the_device_forms_on_a_stream_of_their_own_give_the_bits_of_the_host_forms(built):
    import torch
    from hobbyraytracer_amd import api
    shape, counts = (29, 37), (3, 3, 2)
    n = 29 * 37
    after = synthetic_sums(shape, counts, 77)
    stream = torch.cuda.Stream()
    d_state = torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda")
    d_var = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    assert d_state.data_ptr() % 8 == 0 and api.variance_state_bytes(n) == d_state.numel() * 4
    torch.cuda.synchronize()
    done, state = 0, None
    for buf, c in zip(after, counts):
        d_rgb = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        api.variance_fold_device(n, d_rgb.data_ptr(), done, c, d_state.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(_bits(d_rgb.cpu().numpy()), _bits(buf))                  # the input is only read
        state = api.variance_fold(buf, done, c, state)
        _same_state(d_state.cpu().numpy().reshape(29, 37, 2), state, "fold, device form")
        done += c
    api.variance_finish_device(n, d_state.data_ptr(), done, len(counts), d_var.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    _same(d_var.cpu().numpy().reshape(shape), api.variance_finish(state, done, len(counts)), "finish, device form")
    # the adaptive form, on the null stream too
    r = np.random.default_rng(3)
    count = r.integers(0, 20, n).astype(np.int32)
    sums = (r.uniform(0.1, 2.0, (n, 3)) * count[:, None]).astype(F)
    sq = (r.uniform(0.1, 4.0, n) * count).astype(F)
    host = api.adaptive_variance(sums, sq, count)
    d_sums, d_sq, d_count = torch.from_numpy(sums).cuda(), torch.from_numpy(sq).cuda(), torch.from_numpy(count).cuda()
    torch.cuda.synchronize()
    for s in (stream.cuda_stream, 0):
        d_var.fill_(7.0)
        torch.cuda.synchronize()
        api.adaptive_variance_device(n, d_sums.data_ptr(), d_sq.data_ptr(), d_count.data_ptr(), d_var.data_ptr(), stream=s)
        torch.cuda.synchronize()
        _same(d_var.cpu().numpy(), host, "adaptive, device form")
    # a refused call leaves the device output alone
    with pytest.raises(api.HrtError):
        api.variance_finish_device(n, d_state.data_ptr(), 1, 2, d_var.data_ptr())
    torch.cuda.synchronize()
    _same(d_var.cpu().numpy(), host, "after a refusal")


@pytest.fixture(scope="module")
def cornell(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "cornell_box.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


@pytest.mark.parametrize("flags", [dict(), dict(stratified=True), dict(nee=True)], ids=["default", "stratified", "nee"])
def test_a_real_render_in_batches_of_3_3_2(cornell, flags):
    api, hs, dev = cornell
    W, H, spp = 32, 24, 8
    cam, p = hs.camera(W, H), api.default_params(W, H, spp, seed=5, **flags)
    ranges = api.variance_batches(spp, 3)
    assert ranges == [(0, 3), (3, 3), (6, 2)]
    accum = np.empty((H, W, 3), F)
    state = want = None
    for first, c in ranges:
        dev.render_stripes_accumulate(cam, p, 8, 0, 1, accum, first, c)
        scale = float(spp) if first + c == spp else 1.0
        state = api.variance_fold(accum, first, c, state, scale=scale)
        want = vn.fold(accum, scale, first, c, want)
        _same(state, want, ("state", first))
    var = api.variance_finish(state, spp, 3)
    _same(var, vn.finish(want, spp, 3), "variance of a real render")
    assert np.isfinite(var).all() and (var > 0).any()
    one_shot, _ = dev.render_stripes(cam, p, 8, 0, 1)
    _same(accum, one_shot, "the film in batches against one shot")
    film2, var2 = dev.render_stripes_with_variance(cam, p, batches=3)
    _same(film2, one_shot, "render_stripes_with_variance: film")
    _same(var2, var, "render_stripes_with_variance: variance")
    with pytest.raises(ValueError):
        dev.render_stripes_with_variance(cam, p, batches=1)


def test_the_variance_of_an_adaptive_render_and_the_filter_with_it(cornell):
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
    var = api.adaptive_variance(sums, sq, count)
    _same(var, dn.variance_of_mean_luminance(sums, sq, count), "adaptive variance of a real render")
    film = (sums / count.astype(F)[..., None]).astype(F)
    aov = dev.render_aov_tile(cam, api.default_params(W, H, 8, seed=4))
    raw = np.concatenate([aov["albedo"], aov["alpha"][..., None], aov["normal"], aov["depth"][..., None]], axis=-1)
    _same(api.denoise(film, aov, var, sigma_l=6.0), dn.denoise(film, raw, var, sigma_l=6.0), "the filter with the measured variance")


def test_a_film_rendered_after_variance_calls_is_the_committed_one(built, tmp_path):
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
            p = api.default_params(W, H, spp, quirks=q, seed=11)
            b = want[f"cornell_box_{qn}"]
            film, var = dev.render_stripes_with_variance(cam, p, batches=4)         # 2 + 2 + 2: one rank's stripes are the film
            assert np.array_equal(_bits(film), _bits(b)) and var.shape == (H, W), qn
            api.adaptive_variance(np.ones((5, 3), F), np.ones(5, F), np.full(5, 3, np.int32))
            img, st = dev.render_tile(cam, p)
            same = (img.view(np.uint32) == b.view(np.uint32)) | (np.isnan(img) & np.isnan(b))
            assert same.all(), (qn, int((~same).sum()))
            assert st.rays == int(want[f"cornell_box_{qn}_rays"][0]), qn
    finally:
        dev.close()


def test_cli_measured_variance(cornell, tmp_path, scenes_dir):
    api, hs, dev = cornell
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    W, H, spp = 48, 32, 8
    common = ["s.yaml", "--size", f"{W}x{H}", "--spp", str(spp), "--seed", "2", "--no-progress"]

    def run(*extra):
        return subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=120)

    def pfm(name):
        return api.read_pfm(str(tmp_path / name))

    def aov_of(prefix):
        part = {n: pfm(f"{prefix}.{n}.pfm") for n in ("albedo", "normal", "depth", "alpha")}
        return np.concatenate([part["albedo"], part["alpha"][..., :1], part["normal"], part["depth"][..., :1]], axis=-1)

    cam, p = hs.camera(W, H), api.default_params(W, H, spp, seed=2)
    r = run("--denoise-variance", "measured", "--denoise-batches", "3", "--dump-variance", "var.pfm", "--dump-linear", "filtered.pfm",
            "--dump-noisy", "noisy.pfm", "--aov", "p", "--aov-spp", "4", "--out", "d.png", "--stats")
    assert r.returncode == 1, r.stdout + r.stderr                # Film::outputFilm's 1 = success (Q-12)
    assert "spatial estimate" not in r.stderr
    js = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert js["variance_s"] > 0 and js["denoise_s"] > 0 and js["samples"] == W * H * spp
    film, var = dev.render_stripes_with_variance(cam, p, batches=3)
    got_var = pfm("var.pfm")
    assert np.array_equal(_bits(got_var[..., 0]), _bits(got_var[..., 1])) and np.array_equal(_bits(got_var[..., 0]), _bits(got_var[..., 2]))
    _same(got_var[..., 0], var, "--dump-variance")
    _same(pfm("noisy.pfm"), film, "--dump-noisy")
    aov = aov_of("p")
    _same(pfm("filtered.pfm"), api.denoise(film, aov, var, sigma_l=6.0), "--dump-linear under measured: sigma_l 6")
    r = run("--dump-linear", "plain.pfm", "--out", "n.png")
    assert r.returncode == 1, r.stderr
    assert (tmp_path / "noisy.pfm").read_bytes() == (tmp_path / "plain.pfm").read_bytes()
    # an explicit sigma_l is kept; the default K is 4; --denoise-batches alone implies measured
    r = run("--denoise-batches", "4", "--denoise-sigma-l", "3", "--dump-variance", "var4.pfm", "--dump-linear", "f4.pfm", "--aov-spp", "4", "--out", "e.png")
    assert r.returncode == 1, r.stderr
    film4, var4 = dev.render_stripes_with_variance(cam, p, batches=4)
    _same(pfm("var4.pfm")[..., 0], var4, "K = 4")
    _same(pfm("f4.pfm"), api.denoise(film4, aov, var4, sigma_l=3.0), "an explicit sigma_l")
    r = run("--denoise-variance", "measured", "--dump-variance", "vdef.pfm", "--aov-spp", "4", "--out", "e.png")
    assert r.returncode == 1, r.stderr
    assert (tmp_path / "vdef.pfm").read_bytes() == (tmp_path / "var4.pfm").read_bytes()
    # --progressive: its passes are the batches (3 + 3 + 2)
    r = run("--denoise-variance", "measured", "--progressive", "3", "--dump-variance", "vprog.pfm", "--dump-linear", "fprog.pfm", "--aov-spp", "4", "--out", "g.png")
    assert r.returncode == 1, r.stderr
    assert (tmp_path / "vprog.pfm").read_bytes() == (tmp_path / "var.pfm").read_bytes()
    assert (tmp_path / "fprog.pfm").read_bytes() == (tmp_path / "filtered.pfm").read_bytes()
    # --resume: the resumed sums are the first batch (3, then 3 + 2), and a finished checkpoint leaves nothing to measure from
    r = run("--progressive", "3", "--max-passes", "1", "--checkpoint", "ck.bin", "--out", "c.png")
    assert r.returncode == 1, r.stderr
    r = run("--resume", "--checkpoint", "ck.bin", "--progressive", "3", "--denoise-variance", "measured", "--dump-variance", "vres.pfm",
            "--dump-linear", "fres.pfm", "--aov-spp", "4", "--out", "c.png")
    assert r.returncode == 1, r.stderr
    assert (tmp_path / "vres.pfm").read_bytes() == (tmp_path / "var.pfm").read_bytes()
    assert (tmp_path / "fres.pfm").read_bytes() == (tmp_path / "filtered.pfm").read_bytes()
    r = run("--resume", "--checkpoint", "ck.bin", "--denoise-variance", "measured", "--dump-linear", "fdone.pfm", "--aov-spp", "4", "--out", "c.png")
    assert r.returncode == 1, r.stderr
    assert "spatial estimate" in r.stderr
    _same(pfm("fdone.pfm"), api.denoise(film, aov), "a finished checkpoint: the fallback")
    # spatial is the default and today's bits
    r = run("--denoise-variance", "spatial", "--dump-linear", "fs.pfm", "--aov-spp", "4", "--out", "h.png")
    assert r.returncode == 1, r.stderr
    _same(pfm("fs.pfm"), api.denoise(film, aov), "--denoise-variance spatial")
    # --adaptive: the variance of the adaptive buffers
    r = run("--adaptive", "0.05", "--min-samples", "4", "--progressive", "2", "--denoise-variance", "measured", "--dump-variance", "va.pfm",
            "--dump-linear", "fa.pfm", "--dump-noisy", "na.pfm", "--sample-map", "ca.pfm", "--aov-spp", "4", "--out", "a.png")
    assert r.returncode == 1, r.stderr
    ad = api.Adaptive(4, 2, 0.05, 0.01)
    sums = sq = count = None
    for pass_index in range(8):
        sums, sq, count, active, _ = dev.render_stripes_adaptive(cam, p, 8, 0, 1, ad, pass_index, sums, sq, count)
        if active == 0:
            break
    assert np.array_equal(pfm("ca.pfm")[..., 0], count.astype(F))
    va = api.adaptive_variance(sums, sq, count)
    _same(pfm("va.pfm")[..., 0], va, "--adaptive --dump-variance")
    _same(pfm("fa.pfm"), api.denoise(pfm("na.pfm"), aov, va, sigma_l=6.0), "--adaptive under measured")
    # one sample per pixel: nothing to measure from
    r = subprocess.run([api.CLI_PATH, "s.yaml", "--size", f"{W}x{H}", "--spp", "1", "--seed", "2", "--no-progress", "--denoise-variance", "measured",
                        "--dump-linear", "f1.pfm", "--dump-noisy", "n1.pfm", "--out", "o.png"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stderr
    assert "spatial estimate" in r.stderr
    aov1 = dev.render_aov_tile(cam, api.default_params(W, H, 1, seed=2))
    _same(pfm("f1.pfm"), api.denoise(pfm("n1.pfm"), aov1), "the fallback is the spatial estimate with its own sigma_l")
    # usage errors
    for extra in (("--denoise-variance", "guessed"), ("--denoise-variance",), ("--denoise-batches", "1"), ("--denoise-batches", "65"),
                  ("--denoise-batches", "x"), ("--denoise-batches", "0"), ("--dump-variance", "u.pfm"), ("--denoise", "--dump-variance", "u.pfm"),
                  ("--denoise-variance", "spatial", "--dump-variance", "u.pfm")):
        r = run("--out", "u.png", *extra)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "u.png").exists() and not (tmp_path / "u.pfm").exists()
