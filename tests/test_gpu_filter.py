"""The reconstruction filter (HRT_FLAG_FILTER, include/hrt.h "reconstruction filter") on the GPU: the kernels of
csrc/hrt_filter.hip give the bits of the numpy restatement of the header's words (tests/filter_np.py) -- on synthetic sample stacks of
awkward sizes with every special value, and on real renders, whose per-sample films come from the unfiltered accumulate form; any
batching, the tile and the one-rank stripes agree; a sub-tile is the restatement clipped to it; the counters are the unfiltered
render's and an unfiltered render does not notice a filtered one in front; what cannot be filtered is refused with the output
untouched; and the CLI's --filter writes what the API gives.

Every comparison is of bit patterns; of a NaN only its being one is compared (the header defines no payload)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import filter_np as fn

pytestmark = pytest.mark.gpu
F = np.float32

# (film W, H, rect): whole films -- several blocks with ragged edges; exactly one block; a flat strip, every window clipped above and
# below; one pixel; the smallest film with neighbours -- and a rectangle inside a larger film (the RNG keys are the film's)
RECTS = [(37, 29, None), (16, 16, None), (70, 3, None), (1, 1, None), (2, 2, None), (40, 30, (5, 3, 20, 11))]
# tent at the smallest radius (window half-width 0), its default, and one between two window sizes; the cubics at their default; Mitchell
# at the largest radius; and Mitchell at 1, where single samples leave pixels without a positive weight sum
FILTERS = [("tent", 0.5), ("tent", 1.0), ("tent", 1.7), ("bspline", 2.0), ("mitchell", 2.0), ("mitchell", 2.5), ("mitchell", 1.0), ("bspline", 0.0)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def synthetic(S, h, w, seed):
    """A seeded stack [S, h, w, 3] of sample values with negatives, zeros of both signs, huge and tiny values and, where the stack has
    room, NaN, +Inf and -Inf samples: alone, side by side (Inf - Inf), at the corners and on both sides of the block border at 15 / 16."""
    r = np.random.default_rng(seed)
    rad = (r.uniform(0.0, 2.0, (S, h, w, 1)) * r.uniform(0.2, 1.0, (S, h, w, 3))).astype(F)
    pick = r.random((S, h, w))
    rad[pick < 0.10] = 0.0
    rad[(pick >= 0.10) & (pick < 0.15)] *= F(-1.0)
    rad[(pick >= 0.15) & (pick < 0.17)] = (-0.0, 0.0, -0.0)
    rad[(pick >= 0.17) & (pick < 0.19)] *= F(1e30)
    rad[(pick >= 0.19) & (pick < 0.21)] *= F(1e-38)

    def put(s, x, y, value):
        if s < S and 0 <= x < w and 0 <= y < h:
            rad[s, y, x] = value
    if w * h >= 4:
        put(0, 0, 0, (np.nan, 0.5, 0.25))
        put(S - 1, w - 1, h - 1, (0.5, np.inf, 0.25))
        put(0, w - 1, 0, (0.5, 0.25, -np.inf))
    put(0, 15, 1, (np.inf, 1.0, 1.0)); put(0, 16, 1, (-np.inf, 1.0, 1.0))        # neighbours across a block border: Inf - Inf
    put(S - 1, 8, 15, (np.nan, np.nan, np.nan)); put(S - 1, 8, 16, (1.0, np.inf, -np.inf))
    put(S // 2, 30, 20, (-np.inf, np.nan, np.inf))
    return rad


@pytest.mark.parametrize("case", RECTS, ids=[f"{W}x{H}" + ("" if r is None else "_rect") for W, H, r in RECTS])
def test_the_kernels_give_the_bits_of_the_restatement(built, case):
    from hobbyraytracer_amd import api
    W, H, rect = case
    rect = (0, 0, W, H) if rect is None else rect
    w, h = rect[2:]
    nans = zeros = 0
    for S in (1, 5):
        rad = synthetic(S, h, w, 100 * W + H + S)
        for kind, radius in FILTERS:
            for stratified in (False, True):
                seed = (7 << 32) | (S * 1000 + W)
                want = fn.filter_samples(rad, kind, radius, W, rect, seed, stratified)
                got = api.filter_samples(rad, kind, radius, W, H, rect, seed, stratified)
                _same(got, want, (case, S, kind, radius, stratified))
                nans += int(np.isnan(got).sum())
                zeros += int((fn.weight_sums(S, kind, radius, W, rect, seed, stratified) <= 0).sum()) if (kind, radius, S) == ("mitchell", 1.0, 1) else 0
    if w * h >= 4:                                               # the stacks exercise what they are meant to
        assert nans > 0
    if w * h >= 256:
        assert zeros > 0


def test_a_stack_too_large_for_one_upload_is_gathered_in_batches(built):
    """hrt_filter_samples uploads at most 4 Mi slots at a time: 70 x 64 pixels x 1200 samples are two batches, the second one starting from
    the first one's sums.  Constant samples of a power of two come back exactly wherever the weights sum to something."""
    from hobbyraytracer_amd import api
    W, H, S = 70, 64, 1200
    rad = np.full((S, H, W, 3), 0.5, F)
    got = api.filter_samples(rad, "tent", 1.0, seed=3)
    assert (_bits(got) == _bits(np.full((H, W, 3), 0.5, F))).all()


# ---------------------------------------------------------------- real renders
SCENES = ("cornell_box", "material_zoo")
ESTIMATORS = {"default": {}, "nee": {"nee": True}, "stratified": {"stratified": True}}
RW, RH, RS = 37, 29, 5


@pytest.fixture(scope="module")
def scenes(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    held = {}
    for name in SCENES:
        hs = api.HostScene(os.path.join(scenes_dir, name + ".yaml"), assets)
        held[name] = (hs, api.DeviceScene(hs.flat_ptr, 0))
    yield api, held
    for _, dev in held.values():
        dev.close()


@pytest.fixture(scope="module")
def sample_films(scenes):
    """(scene, estimator) -> [S, H, W, 3]: the value of every sample of every pixel, from the UNFILTERED accumulate form -- a zeroed buffer,
    the range [s, s + 1), and samples = S + 1 in the params so that no call divides.  Computed once, shared, never changed."""
    api, held = scenes
    cache = {}

    def get(scene, est):
        if (scene, est) not in cache:
            hs, dev = held[scene]
            cam, p = hs.camera(RW, RH), api.default_params(RW, RH, RS + 1, seed=11, **ESTIMATORS[est])
            films = np.zeros((RS, RH, RW, 3), F)
            for s in range(RS):
                dev.render_stripes_accumulate(cam, p, 8, 0, 1, films[s], s, 1)
            films.setflags(write=False)
            cache[(scene, est)] = films
        return cache[(scene, est)]
    return get


@pytest.mark.parametrize("est", list(ESTIMATORS))
@pytest.mark.parametrize("scene", SCENES)
def test_a_filtered_render_is_the_restated_gather_of_the_unfiltered_samples(scenes, sample_films, scene, est):
    api, held = scenes
    hs, dev = held[scene]
    films = sample_films(scene, est)
    assert (films > 0).any()
    cam = hs.camera(RW, RH)
    plain, st_plain = dev.render_tile(cam, api.default_params(RW, RH, RS, seed=11, **ESTIMATORS[est]))
    p = api.default_params(RW, RH, RS, seed=11, filter=True, **ESTIMATORS[est])
    for kind, radius in (("mitchell", 0.0), ("tent", 0.0), ("bspline", 0.0), ("tent", 1.7), ("mitchell", 2.5), ("tent", 0.5)):
        dev.set_filter(kind, radius)
        got, st = dev.render_tile(cam, p)
        want = fn.filter_samples(films, kind, radius, RW, (0, 0, RW, RH), 11, est == "stratified")
        _same(got, want, (scene, est, kind, radius))
        assert (st.rays, st.samples, st.shadow_rays) == (st_plain.rays, st_plain.samples, st_plain.shadow_rays), (scene, est, kind)
        assert (_bits(got) != _bits(plain)).any()
    assert st_plain.samples == RW * RH * RS and ((scene, est) != ("cornell_box", "nee") or st_plain.shadow_rays > 0)
    dev.set_filter()


def test_batching_layout_and_sub_tiles(scenes, sample_films):
    api, held = scenes
    hs, dev = held["cornell_box"]
    cam = hs.camera(RW, RH)
    p = api.default_params(RW, RH, RS, seed=11, filter=True)
    for kind, radius in (("mitchell", 0.0), ("tent", 1.0)):
        dev.set_filter(kind, radius)
        one, _ = dev.render_tile(cam, p)
        # accumulate ranges 2 + 2 + 1: the buffer is the unnormalised acc until the call that reaches `samples`
        acc = np.full((RH, RW, 3), 7.0, F)                       # (sample_first == 0 starts it: the buffer need not be cleared)
        dev.render_stripes_accumulate(cam, p, 8, 0, 1, acc, 0, 2)
        films = sample_films("cornell_box", "default")
        _same(acc, fn.accumulate(films[:2], kind, radius, RW, (0, 0, RW, RH), 11), (kind, "acc after [0, 2)"))
        dev.render_stripes_accumulate(cam, p, 8, 0, 1, acc, 2, 2)
        dev.render_stripes_accumulate(cam, p, 8, 0, 1, acc, 4, 1)
        _same(acc, one, (kind, "2 + 2 + 1"))
        # one rank's stripes, whatever the block height, are the tile
        for R in (8, 5):
            stripes, _ = dev.render_stripes(cam, p, R, 0, 1)
            _same(stripes, one, (kind, "stripes", R))
        # a sub-tile: the restatement clipped to it -- pixels outside contribute nothing, so its border differs from the full film's
        rect = (5, 3, 20, 11)
        sub, _ = dev.render_tile(cam, p, rect)
        want = fn.filter_samples(films[:, 3:14, 5:25], kind, radius, RW, rect, 11)
        _same(sub, want, (kind, "sub-tile"))
        inner = one[3:14, 5:25]
        assert (_bits(sub[3:-3, 3:-3]) == _bits(inner[3:-3, 3:-3])).all() and (_bits(sub) != _bits(inner)).any()
    # a one-device session: the same film, in passes too
    dev.set_filter()
    one, _ = dev.render_tile(cam, p)
    ms = api.MultiScene(hs.flat_ptr, devices=(0,))
    try:
        whole, _, st = ms.render(cam, p)
        _same(whole, one, "one-device session")
        ms.set_filter("tent", 1.0)
        dev.set_filter("tent", 1.0)
        a, _, _ = ms.render(cam, p, sample_first=0, sample_count=3)
        b, _, _ = ms.render(cam, p, sample_first=3, sample_count=2)
        _same(b, dev.render_tile(cam, p)[0], "one-device session, 3 + 2")
        assert ms.filter_ms() > 0 and ms.filter_ms() == 0
    finally:
        ms.close()
        dev.set_filter()


def test_an_unfiltered_render_does_not_notice_a_filtered_one_in_front(scenes):
    api, held = scenes
    hs, dev = held["material_zoo"]
    cam = hs.camera(RW, RH)
    p = api.default_params(RW, RH, RS, seed=4, nee=True)
    before, st_before = dev.render_tile(cam, p)
    dev.set_filter("mitchell", 2.5)
    dev.filter_ms()                                             # (reads and clears what the tests before left)
    assert dev.filter_ms() == 0
    filtered, st_f = dev.render_tile(cam, api.default_params(RW, RH, RS, seed=4, nee=True, filter=True))
    assert dev.filter_ms() > 0
    after, st_after = dev.render_tile(cam, p)                   # the scene's filter is set, the flag is not: nothing reads it
    dev.set_filter()
    _same(after, before, "unfiltered after filtered")
    for st in (st_f, st_after):
        assert (st.rays, st.samples, st.shadow_rays) == (st_before.rays, st_before.samples, st_before.shadow_rays)
    assert (_bits(filtered) != _bits(before)).any()
    # the feature buffers accept the flag and stay box-filtered
    a = dev.render_aov_tile(cam, api.default_params(RW, RH, 2, seed=4))
    b = dev.render_aov_tile(cam, api.default_params(RW, RH, 2, seed=4, filter=True))
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_what_cannot_be_filtered_is_refused_with_the_output_untouched(scenes):
    api, held = scenes
    hs, dev = held["cornell_box"]
    W, H = 16, 12
    cam = hs.camera(W, H)
    p = api.default_params(W, H, 4, seed=1, filter=True)
    out = np.full((H, W, 3), 7.0, F)
    sq, count = np.full((H, W), 7.0, F), np.full((H, W), 7, np.int32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    st = api.Stats()

    def refused(status, word):
        assert status == api.HRT_ERR_UNSUPPORTED, (status, word, api._hip.hrt_last_error())
        assert word in api._hip.hrt_last_error().decode(), (word, api._hip.hrt_last_error())
        assert (out == 7.0).all() and (sq == 7.0).all() and (count == 7).all()

    h = dev._h
    for rank in (0, 1):                                         # n_ranks > 1: neighbouring rows belong to other ranks
        refused(api._hip.hrt_render_stripes(h, C.byref(cam), C.byref(p), 4, rank, 2, fp(out), C.byref(st)), "n_ranks")
        refused(api._hip.hrt_render_stripes_accumulate(h, C.byref(cam), C.byref(p), 4, rank, 2, fp(out), 0, 2, C.byref(st)), "n_ranks")
    import torch
    d_out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    refused(api._hip.hrt_render_stripes_device(h, C.byref(cam), C.byref(p), 4, 0, 2, C.c_void_p(d_out.data_ptr()), None), "n_ranks")
    refused(api._hip.hrt_render_stripes_accumulate_device(h, C.byref(cam), C.byref(p), 4, 1, 3, C.c_void_p(d_out.data_ptr()), 0, -1, None), "n_ranks")
    torch.cuda.synchronize()
    assert bool((d_out == 7.0).all())
    # the adaptive entry points: a list of pixels has no neighbours
    ad, active = api.Adaptive(2, 2, 0.05, 0.01), C.c_int64(5)
    refused(api._hip.hrt_render_stripes_adaptive(h, C.byref(cam), C.byref(p), 4, 0, 1, C.byref(ad), fp(out), fp(sq), count.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 0, C.byref(active), C.byref(st)), "adaptive")
    d_sq, d_count = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda"), torch.full((H, W), 7, dtype=torch.int32, device="cuda")
    refused(api._hip.hrt_render_stripes_adaptive_device(h, C.byref(cam), C.byref(p), 4, 0, 1, C.byref(ad), C.c_void_p(d_out.data_ptr()), C.c_void_p(d_sq.data_ptr()),
                                                        C.c_void_p(d_count.data_ptr()), 0, C.byref(active), None), "adaptive")
    torch.cuda.synchronize()
    assert bool((d_out == 7.0).all()) and bool((d_sq == 7.0).all()) and bool((d_count == 7).all())
    # the megakernel
    pm = api.default_params(W, H, 4, seed=1, filter=True, megakernel=True)
    refused(api._hip.hrt_render_tile(h, C.byref(cam), C.byref(pm), api.Rect(0, 0, W, H), fp(out), C.byref(st)), "wavefront")
    refused(api._hip.hrt_render_stripes(h, C.byref(cam), C.byref(pm), 4, 0, 1, fp(out), C.byref(st)), "wavefront")
    # a session of more than one device, loopback included
    ms = api.MultiScene(hs.flat_ptr, devices=(0, 0), loopback=True)
    try:
        ms.set_filter("bspline")
        u8 = np.full((H, W, 3), 7, np.uint8)
        refused(api._hip.hrt_multi_render(ms._h, C.byref(cam), C.byref(p), 4, 0, -1, None, fp(out), u8.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st)), "one device")
        assert (u8 == 7).all()
        plain, _, _ = ms.render(cam, api.default_params(W, H, 4, seed=1))     # without the flag the session renders as ever
        _same(plain, dev.render_tile(cam, api.default_params(W, H, 4, seed=1))[0], "two ranks, unfiltered")
    finally:
        ms.close()
    # the setters on live handles: a refused value leaves what was set
    dev.set_filter("tent", 1.5)
    with pytest.raises(api.HrtError) as e:
        dev.set_filter("tent", 2.6)
    assert e.value.status == api.HRT_ERR_INVALID
    with pytest.raises(api.HrtError):
        dev.set_filter(5, 1.0)
    kept, _ = dev.render_tile(cam, p)
    dev.set_filter("tent", 1.5)
    _same(dev.render_tile(cam, p)[0], kept, "a refused setter changes nothing")
    dev.set_filter()


def test_cli_filter(scenes, tmp_path, scenes_dir):
    api, held = scenes
    hs, dev = held["cornell_box"]
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    W, H, spp = 48, 32, 6
    common = ["s.yaml", "--size", f"{W}x{H}", "--spp", str(spp), "--seed", "2", "--no-progress"]

    def run(*extra):
        return subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=120)

    cam = hs.camera(W, H)
    r0 = run("--dump-linear", "plain.pfm", "--out", "p.png", "--stats")
    assert r0.returncode == 1, r0.stdout + r0.stderr            # Film::outputFilm's 1 = success (Q-12)
    js0 = json.loads([ln for ln in r0.stdout.splitlines() if ln.startswith("{")][-1])
    assert "filter" not in js0 and "filter_s" not in js0
    for extra, setting, kw in ((("--filter", "mitchell"), ("mitchell", 0.0), {}),
                               (("--filter", "tent", "--filter-radius", "1.5", "--nee", "--stratified", "--roulette", "--progressive", "4"), ("tent", 1.5),
                                {"nee": True, "stratified": True, "roulette": True})):
        r = run(*extra, "--dump-linear", "f.pfm", "--out", "f.png", "--stats")
        assert r.returncode == 1, r.stdout + r.stderr
        dev.set_filter(*setting)
        want, st = dev.render_tile(cam, api.default_params(W, H, spp, seed=2, filter=True, **kw))
        got = api.read_pfm(str(tmp_path / "f.pfm"))
        _same(got, want, extra)
        assert np.array_equal(api.read_png(str(tmp_path / "f.png")), dev.resolve_u8(want))
        js = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert js["filter"] == setting[0] and js["filter_s"] > 0 and js["samples"] == W * H * spp
        if not kw:
            assert js["rays"] == js0["rays"] == st.rays
    dev.set_filter()
    # ahead of the post-render stages: they take the filtered film
    r = run("--filter", "mitchell", "--despeckle", "--denoise", "--dump-noisy", "n.pfm", "--dump-linear", "d.pfm", "--aov", "a", "--out", "d.png")
    assert r.returncode == 1, r.stdout + r.stderr
    want, _ = dev.render_tile(cam, api.default_params(W, H, spp, seed=2, filter=True))
    _same(api.read_pfm(str(tmp_path / "n.pfm")), want, "--dump-noisy under --filter")
    assert (_bits(api.read_pfm(str(tmp_path / "d.pfm"))) != _bits(want)).any()
    r2 = run("--aov", "b", "--out", "b.png")
    assert r2.returncode == 1
    for part in ("albedo", "normal", "depth", "alpha"):          # the feature buffers stay box-filtered
        assert (tmp_path / f"a.{part}.pfm").read_bytes() == (tmp_path / f"b.{part}.pfm").read_bytes()
    # usage errors (exit 2, nothing written)
    for extra in (("--filter-radius", "1.5"), ("--filter", "gauss"), ("--filter", "mitchell", "--adaptive", "0.05"), ("--filter", "mitchell", "--gpus", "2"),
                  ("--filter", "tent", "--checkpoint", "c.ckpt"), ("--filter", "tent", "--denoise-batches", "3"),
                  ("--filter", "tent", "--denoise-variance", "measured")):
        r = run(*extra, "--out", "u.png")
        assert r.returncode == 2 and not (tmp_path / "u.png").exists(), (extra, r.returncode, r.stderr)
