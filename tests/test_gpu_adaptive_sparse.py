"""Adaptive sampling's sparse passes (RenderMap mode 2) at every list shape and for every estimator.

The test chooses the active set S itself: with threshold 0 a pixel is active in pass k >= 1 exactly when count == done, so
tests/adaptive_np.py crafts buffers that hold `done` and the uniform render's running sums in S and sentinels (NaNs, counts that never
match) everywhere else.  One pass must then return, bit for bit, the uniform accumulation after done + n samples in S (sums, the float32
running sum of Y*Y in sq, count) and the inputs' bits outside S; active == |S| and Stats.samples == |S| * n.  The reference is the
uniform path (hrt_render_stripes_accumulate one sample at a time), which the parity and *_f64 tests pin to the oracle and to float64.
A dropped pixel, a duplicated one, a slot divided by the wrong list length or a per-slot buffer indexed by pixel shows as a difference."""
import os

import numpy as np
import pytest

from tests import adaptive_np as ad
from tests.test_gpu_adaptive import _luma, _rule
from tests.test_gpu_nee_lobes import FOG_ROOM_YAML, _scene
from tests.test_gpu_stratified import MIXED_LIGHTS_YAML

pytestmark = pytest.mark.gpu

SEED = 11          # of every render here (not the default 0)


def _reference(api, dev, hs, W, H, R, rank, G, spp, flags=None, check_at=()):
    """The uniform render's per-sample radiance of one rank's stripes (spp single-sample accumulate calls; params.samples = spp + 1
    keeps them from dividing) and the float32 running sums and running sums of Y*Y built from it.  check_at: sample counts at which
    the running sums are compared with the ones longer accumulate calls leave in one buffer."""
    flags = flags or {}
    cam = hs.camera(W, H)
    pu = api.default_params(W, H, spp + 1, seed=SEED, **flags)
    rows = api.stripe_rows(H, R, rank, G)
    rad = np.empty((spp, rows, W, 3), np.float32)
    for s in range(spp):
        acc = np.zeros((rows, W, 3), np.float32)
        dev.render_stripes_accumulate(cam, pu, R, rank, G, acc, s, 1)
        rad[s] = acc
    prefix = ad.sum_prefix(rad)
    acc, at = np.zeros((rows, W, 3), np.float32), 0
    for n in sorted(check_at):
        dev.render_stripes_accumulate(cam, pu, R, rank, G, acc, at, n - at)
        at = n
        assert ad.same_bits(acc, prefix[n]), f"the running sums after {n} samples are not the float32 sums of the single samples"
    return dict(cam=cam, p=api.default_params(W, H, spp, seed=SEED, **flags), rows=rows, W=W, R=R, rank=rank, G=G, spp=spp,
                rad=rad, prefix=prefix, y2=ad.y2_prefix(rad))


def _differences(label, got, want, S):
    """what differs between the buffers a pass returned and the expected ones -> list of lines (empty: bit-equal)"""
    lines = []
    for name, g, w in zip(("sums", "sq", "count"), got, want):
        if not ad.same_bits(g, w):
            bad = g.view(np.uint32) != w.view(np.uint32)
            bad = (bad.any(-1) if bad.ndim == 3 else bad).ravel()
            q = np.flatnonzero(bad)
            lines.append(f"{label}: {name} differs at {q.size} pixels ({int(S.ravel()[q].sum())} of them in S, |S| = {int(S.sum())}), "
                         f"first {q[:6].tolist()}: got {g.reshape(bad.size, -1)[q[:2]].tolist()}, want {w.reshape(bad.size, -1)[q[:2]].tolist()}")
    return lines


def _crafted_pass(dev, ref, adaptive, k, S, seed, label, inputs=None):
    """Pass k >= 1 of `adaptive` (threshold 0) on the active set S -> (lines of what is wrong, the buffers returned, Stats)."""
    done = adaptive.min_samples + (k - 1) * adaptive.pass_samples
    n = min(adaptive.pass_samples, ref["spp"] - done)
    assert adaptive.threshold == 0.0 and k >= 1 and n >= 1
    shape = (ref["rows"], ref["W"])
    S = ad.as_mask(S, shape)
    if inputs is None:
        inputs = ad.crafted(ref["prefix"][done], ref["y2"][done], S, done, seed)
    assert np.array_equal(inputs[2] == done, S)
    want = ad.expect(inputs, ref["prefix"][done + n], ref["y2"][done + n], S, done, n)
    sums, sq, count, active, st = dev.render_stripes_adaptive(ref["cam"], ref["p"], ref["R"], ref["rank"], ref["G"], adaptive, k,
                                                              *[a.copy() for a in inputs])
    lines = _differences(label, (sums, sq, count), want, S)
    if active != S.sum():
        lines.append(f"{label}: active = {active}, |S| = {int(S.sum())}")
    if st.samples != int(S.sum()) * n:
        lines.append(f"{label}: Stats.samples = {st.samples}, |S| * n = {int(S.sum()) * n}")
    if not (count >= inputs[2]).all():
        lines.append(f"{label}: count decreased at {int((count < inputs[2]).sum())} pixels")
    return lines, (sums, sq, count), st


class _Cornell:
    def __init__(self, api, hs, dev):
        self.api, self.hs, self.dev = api, hs, dev
        self._refs = {}

    def ref(self, film, spp):
        """the reference of one film (W, H, R, rank, G), rendered once per (film, spp)"""
        if (film, spp) not in self._refs:
            self._refs[film, spp] = _reference(self.api, self.dev, self.hs, *film, spp, check_at=(spp,))
        return self._refs[film, spp]


@pytest.fixture(scope="module")
def cornell(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "cornell_box.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield _Cornell(api, hs, dev)
    dev.close()


@pytest.fixture(autouse=True)
def _default_pipeline(monkeypatch):
    """every test starts from the pipeline's own batch size and tail round"""
    monkeypatch.delenv("HRT_WF_MAX_SLOTS", raising=False)
    monkeypatch.delenv("HRT_WF_TAIL_ROUND", raising=False)


# ---------------------------------------------------------------- the compaction at every list shape (default estimator, Cornell)

FILMS = [(520, 512, 8, 0, 1),      # 266 240 local pixels = 260 compaction blocks: past k_ad_scan's 256-entry chunk
         (37, 29, 8, 0, 1),        # 1073 pixels: two blocks, the second nearly empty; width no multiple of 8 or 64
         (37, 21, 8, 0, 3), (37, 21, 8, 1, 3), (37, 21, 8, 2, 3),      # rows 8, 8, 5: slot_pixel's row-block arithmetic through the list
         (5, 3, 8, 0, 1), (2, 2, 8, 0, 1)]                             # fewer pixels than one wave (2 x 2: the smallest film the library renders)
SMALL = (37, 29, 8, 0, 1)


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "x".join(map(str, f[:2])) + f"-rank{f[3]}of{f[4]}")
def test_one_pass_renders_exactly_the_chosen_set(cornell, film):
    """Adaptive(2, 1, 0, 0), pass 1 (done = 2, one sample) on every active set of adaptive_np.patterns the film has room for."""
    c = cornell
    ref = c.ref(film, 3)
    n_local = ref["rows"] * ref["W"]
    assert ref["rows"] == {(37, 21, 8, 2, 3): 5, (37, 21, 8, 0, 3): 8, (37, 21, 8, 1, 3): 8}.get(film, film[1])
    sets = ad.patterns(n_local, seed=n_local)
    assert {"empty", "first_pixel", "last_pixel", "all", "first_1", "last_1", "random_three"} <= set(sets)
    if film == FILMS[0]:
        assert n_local == 260 * ad.AD_ITEMS
        assert {"block_255", "block_256", "blocks_255_and_256", "blocks_from_256", "all_but_block_0", "one_per_block", "first_1025",
                "last_1025", "mod1024_is_0", "mod1024_is_1023", "mod64_is_63", "random_half", "random_hundredth"} <= set(sets)
    if film == SMALL:
        assert {"first_1025", "last_1025", "mod1024_is_0", "mod1024_is_1023", "mod64_is_63", "all_but_block_0", "one_per_block"} <= set(sets)
    adaptive = c.api.Adaptive(2, 1, 0.0, 0.0)
    lines = []
    for i, (name, idx) in enumerate(sets.items()):
        assert idx.size == ad.pattern_sizes(n_local)[name]
        wrong, out, st = _crafted_pass(c.dev, ref, adaptive, 1, idx, seed=100 + i, label=name)
        lines += wrong
    assert not lines, "\n".join(lines[:40])


def test_a_rank_without_rows_has_nothing_to_do(cornell):
    c = cornell
    W, H, R, rank, G = 16, 8, 8, 2, 3
    assert c.api.stripe_rows(H, R, rank, G) == 0
    cam, p = c.hs.camera(W, H), c.api.default_params(W, H, 3, seed=SEED)
    for k in (0, 1):
        sums, sq, count, active, st = c.dev.render_stripes_adaptive(cam, p, R, rank, G, c.api.Adaptive(2, 1, 0.0, 0.0), k,
                                                                    np.empty((0, W, 3), np.float32), np.empty((0, W), np.float32),
                                                                    np.empty((0, W), np.int32))
        assert active == 0 and st.samples == 0 and sums.size == sq.size == count.size == 0


def test_a_film_of_one_pixel_is_refused_with_the_buffers_untouched(cornell):
    """1 x 1: every render entry point refuses a film below 2 x 2 (the camera divides by W - 1 and H - 1), the adaptive one too, in
    pass 0 and in a later pass, and leaves the buffers alone."""
    c = cornell
    api = c.api
    cam, p = c.hs.camera(2, 2), api.default_params(1, 1, 3, seed=SEED)
    with pytest.raises(api.HrtError) as e:
        c.dev.render_stripes_accumulate(cam, api.default_params(1, 1, 4, seed=SEED), 8, 0, 1, np.zeros((1, 1, 3), np.float32), 0, 1)
    assert e.value.status == api.HRT_ERR_INVALID
    for k in (0, 1):
        bufs = (np.full((1, 1, 3), np.nan, np.float32), np.full((1, 1), 7.0, np.float32), np.full((1, 1), 2, np.int32))
        keep = [a.copy() for a in bufs]
        with pytest.raises(api.HrtError) as e:
            c.dev.render_stripes_adaptive(cam, p, 8, 0, 1, api.Adaptive(2, 1, 0.0, 0.0), k, *bufs)
        assert e.value.status == api.HRT_ERR_INVALID
        assert all(ad.same_bits(a, b) for a, b in zip(bufs, keep))


@pytest.mark.parametrize("tail_round", ["1", "1000"], ids=["wavefront-tail", "wavefront-rounds"])
def test_both_regimes_of_the_default_pipeline_see_a_sparse_list(cornell, monkeypatch, tail_round):
    """k_wf_tail from round 1 on, and the per-round kernels to the end, as tests/test_gpu_scenes.py selects them."""
    c = cornell
    ref = c.ref(SMALL, 3)
    monkeypatch.setenv("HRT_WF_TAIL_ROUND", tail_round)
    idx = ad.patterns(ref["rows"] * ref["W"], seed=1)["random_half"]
    lines, _, _ = _crafted_pass(c.dev, ref, c.api.Adaptive(2, 1, 0.0, 0.0), 1, idx, seed=7, label=f"tail round {tail_round}")
    assert not lines, "\n".join(lines)


def test_two_passes_render_what_is_left_of_the_first_set(cornell):
    """Adaptive(2, 2, 0, 0) at 6 spp: pass 1 on a random S1; the host then takes a random half of S1 out (a count that does not
    match); pass 2 renders exactly the other half.  Nothing outside S1 ever changes and no count ever decreases."""
    c = cornell
    ref = c.ref(SMALL, 6)
    shape = (ref["rows"], ref["W"])
    n_local = shape[0] * shape[1]
    adaptive = c.api.Adaptive(2, 2, 0.0, 0.0)
    rng = np.random.default_rng(21)
    S1 = np.sort(rng.choice(n_local, n_local // 2, replace=False))
    first = ad.crafted(ref["prefix"][2], ref["y2"][2], S1, 2, seed=22)
    lines, out1, _ = _crafted_pass(c.dev, ref, adaptive, 1, S1, seed=None, label="pass 1", inputs=first)
    assert not lines, "\n".join(lines)
    assert (out1[2].ravel()[S1] == 4).all()
    stopped = rng.permutation(S1)[: S1.size // 2]
    S2 = np.setdiff1d(S1, stopped)
    assert 0 < S2.size < S1.size
    second = tuple(a.copy() for a in out1)
    second[2].reshape(-1)[stopped] = rng.choice(ad.other_counts(4), stopped.size)
    lines, out2, _ = _crafted_pass(c.dev, ref, adaptive, 2, S2, seed=None, label="pass 2", inputs=second)
    assert not lines, "\n".join(lines)
    M1, M2 = ad.as_mask(S1, shape), ad.as_mask(S2, shape)
    for a, b in zip(out2, first):
        assert ad.same_bits(a[~M1], b[~M1])                      # outside S1: the very first inputs, sentinels and NaNs included
    assert ad.same_bits(out2[0][M2], ref["prefix"][6][M2]) and ad.same_bits(out2[1][M2], ref["y2"][6][M2]) and (out2[2][M2] == 6).all()
    half = M1 & ~M2
    assert ad.same_bits(out2[0][half], ref["prefix"][4][half]) and ad.same_bits(out2[1][half], ref["y2"][4][half])
    # pass 3: every pixel left is at 6 = samples
    out3 = c.dev.render_stripes_adaptive(ref["cam"], ref["p"], 8, 0, 1, adaptive, 3, *[a.copy() for a in out2])
    assert out3[3] == 0 and out3[4].samples == 0 and all(ad.same_bits(a, b) for a, b in zip(out3[:3], out2))


def test_a_list_pass_in_sample_chunks_gives_the_bits_of_one_batch(cornell, monkeypatch):
    """HRT_WF_MAX_SLOTS = 2 |S|: the five samples of a pass as 2 + 2 + 1 (the chunks after the first continue the sums the one
    before wrote); pass 0 over NaN-filled buffers as 2 + 2 + 1 too (its first chunk reads nothing)."""
    c = cornell
    ref = c.ref(SMALL, 7)
    shape = (ref["rows"], ref["W"])
    n_local = shape[0] * shape[1]
    idx = ad.patterns(n_local, seed=2)["random_half"]
    adaptive = c.api.Adaptive(2, 5, 0.0, 0.0)
    lines, whole, st = _crafted_pass(c.dev, ref, adaptive, 1, idx, seed=31, label="one batch")
    assert not lines, "\n".join(lines)
    monkeypatch.setenv("HRT_WF_MAX_SLOTS", str(2 * idx.size))
    lines, chunked, st = _crafted_pass(c.dev, ref, adaptive, 1, idx, seed=31, label="2 + 2 + 1")
    assert not lines, "\n".join(lines)
    assert all(ad.same_bits(a, b) for a, b in zip(chunked, whole))
    # pass 0
    first = c.api.Adaptive(5, 1, 0.0, 0.0)

    def pass0():
        out = c.dev.render_stripes_adaptive(ref["cam"], ref["p"], 8, 0, 1, first, 0, np.full(shape + (3,), np.nan, np.float32),
                                            np.full(shape, np.nan, np.float32), np.full(shape, -7, np.int32))
        assert out[3] == n_local and out[4].samples == n_local * 5
        return out[:3]
    monkeypatch.setenv("HRT_WF_MAX_SLOTS", str(2 * n_local))
    chunked = pass0()
    monkeypatch.delenv("HRT_WF_MAX_SLOTS")
    whole = pass0()
    assert all(ad.same_bits(a, b) for a, b in zip(chunked, whole))
    everything = np.ones(shape, np.bool_)
    want = (ref["prefix"][5], ref["y2"][5], np.full(shape, 5, np.int32))
    assert not _differences("pass 0 in chunks", chunked, want, everything)


def test_the_device_form_gives_the_host_forms_bits(cornell):
    """hrt_render_stripes_adaptive_device on torch buffers, on a stream of its own, for a sparse set."""
    import torch
    c = cornell
    ref = c.ref(SMALL, 3)
    shape = (ref["rows"], ref["W"])
    idx = ad.patterns(shape[0] * shape[1], seed=3)["random_hundredth"]
    adaptive = c.api.Adaptive(2, 1, 0.0, 0.0)
    inputs = ad.crafted(ref["prefix"][2], ref["y2"][2], idx, 2, seed=41)
    lines, host, _ = _crafted_pass(c.dev, ref, adaptive, 1, idx, seed=None, label="host form", inputs=inputs)
    assert not lines, "\n".join(lines)
    stream = torch.cuda.Stream()
    sums, sq, count = (torch.from_numpy(a.copy()).cuda() for a in inputs)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        active = c.dev.render_stripes_adaptive_device(ref["cam"], ref["p"], 8, 0, 1, adaptive, sums.data_ptr(), sq.data_ptr(), count.data_ptr(),
                                                      1, stream.cuda_stream)
    stream.synchronize()
    assert active == idx.size
    got = (sums.cpu().numpy(), sq.cpu().numpy(), count.cpu().numpy())
    assert not _differences("device form", got, host, ad.as_mask(idx, shape))
    c.dev.stats()


# ---------------------------------------------------------------- every estimator on a sparse list

_NEE_ALL = dict(nee_lobes=True, nee_env=True, nee_emitters=True)
FLAGS = {"plain": {}, "nee": dict(nee=True), "nee_env": dict(nee_env=True), "nee_emitters": dict(nee_emitters=True),
         "nee_lobes": dict(nee_lobes=True), "nee_all": _NEE_ALL, "stratified": dict(stratified=True), "roulette": dict(roulette=True),
         "all": dict(stratified=True, roulette=True, **_NEE_ALL)}
# the flag set whose film each one must differ from: the same call without the flag(s) the case is about
WITHOUT = {"nee": "plain", "nee_env": "nee", "nee_emitters": "nee", "nee_lobes": "nee", "nee_all": "nee", "stratified": "plain",
           "roulette": "plain", "all": "nee_all"}
# ... and, for the roulette sets, the same estimator without roulette (more rays)
NO_ROULETTE = {"roulette": {}, "all": dict(stratified=True, **_NEE_ALL)}

ESTIMATOR_CASES = [("cornell_box", "plain", 0, 1), ("cornell_box", "nee", 0, 1), ("cornell_box", "stratified", 0, 1),
                   ("cornell_box", "roulette", 0, 1), ("fog_room", "nee_lobes", 0, 1), ("mixed_lights", "nee_emitters", 0, 1),
                   ("teapot_scene", "nee_env", 0, 1), ("teapot_scene", "nee_all", 0, 1), ("teapot_scene", "all", 0, 1),
                   ("teapot_scene", "all", 1, 3), ("three_meshes", "plain", 0, 1), ("three_meshes", "nee", 0, 1)]


@pytest.fixture(scope="module")
def scenes(built, assets, scenes_dir, tmp_path_factory):
    from hobbyraytracer_amd import api
    d = tmp_path_factory.mktemp("sparse_scenes")
    host = {name: api.HostScene(os.path.join(scenes_dir, name + ".yaml"), assets) for name in ("cornell_box", "teapot_scene", "three_meshes")}
    host["fog_room"] = _scene(d, "fog_room", FOG_ROOM_YAML)
    host["mixed_lights"] = _scene(d, "mixed_lights", MIXED_LIGHTS_YAML)
    device = {}

    def get(name):
        if name not in device:
            device[name] = api.DeviceScene(host[name].flat_ptr, 0)
        return host[name], device[name]
    yield api, get
    for dev in device.values():
        dev.close()


@pytest.mark.parametrize("scene,flag_set,rank,G", ESTIMATOR_CASES, ids=lambda v: str(v))
def test_every_estimator_on_a_sparse_list(scenes, scene, flag_set, rank, G):
    """Film 40 x 36 in row blocks of 4, Adaptive(4, 4, 0, 0) at 12 spp: pass 1 on a random S of density 0.3 (done = 4), pass 2 on a
    random half of it (done = 8), each from crafted buffers."""
    api, get = scenes
    hs, dev = get(scene)
    W, H, R, spp = 40, 36, 4, 12
    flags = FLAGS[flag_set]
    roulette = flags.get("roulette", False)
    if roulette:
        dev.set_roulette(0, 0.2)             # ends paths from the first vertex on
    try:
        ref = _reference(api, dev, hs, W, H, R, rank, G, spp, flags, check_at=(4, 8, 12))
        cam, p = ref["cam"], ref["p"]
        assert ref["rows"] == (36 if G == 1 else 12)
        # the method: the one-shot uniform film is the running sum of the twelve single samples, divided
        film, st_film = dev.render_stripes(cam, p, R, rank, G)
        assert ad.same_bits(film, ref["prefix"][spp] / np.float32(spp))
        assert np.isfinite(film).all() and film.max() > 0
        # the flags do something in this scene
        if flag_set in WITHOUT:
            other, _ = dev.render_stripes(cam, api.default_params(W, H, spp, seed=SEED, **FLAGS[WITHOUT[flag_set]]), R, rank, G)
            assert not np.array_equal(film, other), f"{flag_set} renders the film of {WITHOUT[flag_set]} in {scene}"
        if scene == "three_meshes":
            assert hs.flat_ptr.contents.n_meshes > 1         # k_wf_pre runs
        if roulette:
            _, st_no = dev.render_stripes(cam, api.default_params(W, H, spp, seed=SEED, **NO_ROULETTE[flag_set]), R, rank, G)
            assert st_film.rays < st_no.rays
        n_local = ref["rows"] * W
        rng = np.random.default_rng(51 + rank)
        S1 = np.sort(rng.choice(n_local, int(round(0.3 * n_local)), replace=False))
        S2 = np.sort(rng.permutation(S1)[: S1.size // 2])
        adaptive = api.Adaptive(4, 4, 0.0, 0.0)
        lines = []
        for k, S in ((1, S1), (2, S2)):
            wrong, _, st = _crafted_pass(dev, ref, adaptive, k, S, seed=60 + k, label=f"{scene} {flag_set} pass {k}")
            lines += wrong
            if any(key.startswith("nee") for key in flags):
                assert st.shadow_rays > 0, (scene, flag_set, k)
            else:
                assert st.shadow_rays == 0
        assert not lines, "\n".join(lines)
    finally:
        if roulette:
            dev.set_roulette()


# ---------------------------------------------------------------- the stopping rule on estimator samples

@pytest.mark.parametrize("flag_set", ["nee", "stratified", "all"])
def test_natural_threshold_keeps_the_prefix_property(cornell, flag_set):
    """64 x 64 Cornell at 32 spp, Adaptive(8, 8, thr, 0.01) with the first thr that leaves both stopped and unstopped pixels: the
    checks of test_gpu_adaptive.py::test_prefix_property_sq_and_stopping_decisions on the estimators' samples."""
    c = cornell
    api, dev = c.api, c.dev
    W = H = 64
    spp, mn, ps, floor = 32, 8, 8, 0.01
    flags = FLAGS[flag_set]
    roulette = flags.get("roulette", False)
    if roulette:
        dev.set_roulette(0, 0.2)
    try:
        ref = _reference(api, dev, c.hs, W, H, 8, 0, 1, spp, flags, check_at=(8, 16, 24, 32))
        cam, p = ref["cam"], ref["p"]
        for thr in (0.02, 0.04, 0.08, 0.15, 0.3):
            sums = sq = count = None
            k = samples = shadow = 0
            while True:
                sums, sq, count, active, st = dev.render_stripes_adaptive(cam, p, 8, 0, 1, api.Adaptive(mn, ps, thr, floor), k, sums, sq, count)
                samples += st.samples
                shadow += st.shadow_rays
                if active == 0:
                    break
                k += 1
            if (count < spp).any() and (count == spp).any():
                break
        else:
            pytest.fail("no threshold gave both stopped and unstopped pixels")
        assert set(np.unique(count)) <= set(range(mn, spp + 1, ps))
        assert samples == count.sum()
        if flag_set != "stratified":
            assert shadow > 0
        prefix, sq_prefix = ref["prefix"], ref["y2"]
        iy, ix = np.indices(count.shape)
        assert ad.same_bits(sums, prefix[count, iy, ix])
        assert ad.same_bits(sq, sq_prefix[count, iy, ix])
        assert np.array_equal(_luma(ref["rad"]), ad.luma(ref["rad"]))
        # the decision that ended each pixel ...
        stopped = count < spp
        lhs, rhs, slack = _rule(sums, sq, count, thr, floor)
        clear = np.abs(lhs - rhs) > slack
        assert (lhs[stopped & clear] < rhs[stopped & clear]).all()
        n_stopped_clear = (stopped & clear).sum()
        # ... and the one before it kept the pixel going
        went_on = count > mn
        prev = np.maximum(count - ps, mn)
        lhs, rhs, slack = _rule(prefix[prev, iy, ix], sq_prefix[prev, iy, ix], prev, thr, floor)
        clear = np.abs(lhs - rhs) > slack
        assert not (lhs[went_on & clear] < rhs[went_on & clear]).any()
        assert n_stopped_clear > 0 and (went_on & clear).sum() > 0
        print(f"cornell 64x64x{spp} {flag_set}, threshold {thr}: {k} passes, {samples} samples = {samples / count.size / spp:.3f} of uniform")
    finally:
        if roulette:
            dev.set_roulette()
