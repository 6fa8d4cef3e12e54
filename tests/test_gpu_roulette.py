"""Russian roulette (HRT_FLAG_ROULETTE) on the GPU: the film is unbiased against the default estimator's (block means,
z-scores) with and without the NEE flags and the stratified sampler, for the default parameters and for roulette from the first vertex;
every tiling, striping, batching, adaptive and multi-GPU form gives the same bits; the megakernel and HRT_FLAG_STATS refuse it; the CLI
renders with its three switches and keeps its checkpoints apart by flag and by parameters; without the flag the film and the segment count
are the committed ones; and with it far fewer segments are traced."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_stratified import _block_stats, _five_scenes

pytestmark = pytest.mark.gpu

# What tests/tools/roulette_time.py --segments measured: st.rays with the flag (default parameters: first_bounce 3,
# q_floor 0.05) / st.rays without it, seed 0, and the standard deviation of that ratio over the seeds 0..7.
#   cornell_box.yaml 256 x 256, 64 spp, --nee            teapot_scene.yaml 640 x 640, 100 spp (the headline frame's stand-in assets)
SEGMENTS_MEASURED = {"cornell_box": (0.4273, 0.00021), "teapot_scene": (0.3773, 0.00008)}
# st.rays of the same two frames WITHOUT the flag, seed 0: the counts of the commit before this flag existed, which the flag off must keep
SEGMENTS_WITHOUT = {"cornell_box": 31260209, "teapot_scene": 342723490}


def _report(line):
    """measurements (DESIGN.md 4.10 quotes them); shown by pytest -s"""
    print(line)


FLAG_SETS = {"plain": dict(), "nee": dict(nee=True), "nee_all": dict(nee_lobes=True, nee_env=True, nee_emitters=True), "stratified": dict(stratified=True)}
PARAM_SETS = {"default": (3, 0.05), "from_vertex_0": (0, 0.05)}


@pytest.mark.parametrize("flags", list(FLAG_SETS), ids=list(FLAG_SETS))
def test_roulette_is_unbiased(built, assets, scenes_dir, tmp_path, flags):
    """max |z| of the 16 x 16 block means against the default estimator, 16 seeds x 16 spp on 64 x 64 (tests/test_gpu_stratified.py's method)"""
    from hobbyraytracer_amd import api
    W = H = 64
    seeds, spp = 16, 16
    kw = FLAG_SETS[flags]
    for name, hs in _five_scenes(assets, scenes_dir, tmp_path).items():
        dev = api.DeviceScene(hs.flat_ptr, 0)
        try:
            cam = hs.camera(W, H)
            base, rays0 = [], 0
            for s in range(seeds):
                img, st = dev.render_tile(cam, api.default_params(W, H, spp, seed=1000 + s, **kw))   # reference quirks
                base.append(img.astype(np.float64)); rays0 += st.rays
            ma, sa = _block_stats(np.array(base))
            for pname, (first, floor) in PARAM_SETS.items():
                dev.set_roulette(first, floor)
                films, rays1 = [], 0
                for s in range(seeds):
                    img, st = dev.render_tile(cam, api.default_params(W, H, spp, seed=1000 + s, roulette=True, **kw))
                    films.append(img.astype(np.float64)); rays1 += st.rays
                assert not np.array_equal(films[0], base[0]), (name, pname)           # the flag ends paths
                assert rays1 < rays0, (name, pname, rays1, rays0)
                mb, sb = _block_stats(np.array(films))
                z = (mb - ma) / np.sqrt(sa * sa + sb * sb + 1e-30)
                _report(f"{name} {flags} {pname}: max |z| of 16x16 block means roulette vs default = {np.abs(z).max():.2f}; "
                        f"mean block std error default {sa.mean():.4g}, roulette {sb.mean():.4g}; segments {rays1 / rays0:.4f} of the default's")
                assert np.abs(z).max() < 5.0, (name, pname, z)
        finally:
            dev.close()


@pytest.fixture(scope="module")
def cornell(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "cornell_box.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


@pytest.mark.parametrize("params", [(3, 0.05), (1, 0.2)], ids=["default", "start1_floor0.2"])
@pytest.mark.parametrize("stratified", [False, True], ids=["philox", "stratified"])
def test_roulette_forms_agree_bit_for_bit(cornell, params, stratified):
    api, hs, dev = cornell
    W, H, spp = 48, 40, 6
    cam = hs.camera(W, H)
    dev.set_roulette(*params)
    try:
        p = api.default_params(W, H, spp, seed=3, nee=True, stratified=stratified, roulette=True)
        tile, st = dev.render_tile(cam, p)
        assert st.shadow_rays > 0
        plain, st_plain = dev.render_tile(cam, api.default_params(W, H, spp, seed=3, nee=True, stratified=stratified))
        assert not np.array_equal(tile, plain) and st.rays < st_plain.rays and st.shadow_rays < st_plain.shadow_rays
        # tiles: four rectangles of unequal size
        film, rays = np.zeros_like(tile), 0
        for x0, y0, w, h in ((0, 0, 17, 9), (17, 0, 31, 9), (0, 9, 30, 31), (30, 9, 18, 31)):
            part, sp = dev.render_tile(cam, p, (x0, y0, w, h))
            film[y0:y0 + h, x0:x0 + w] = part; rays += sp.rays
        assert np.array_equal(film.view(np.uint32), tile.view(np.uint32)) and rays == st.rays
        # stripes of 1, 2, 3 and 4 ranks (rank 1 of 3 among them)
        for G in (1, 2, 3, 4):
            film, rays = np.zeros_like(tile), 0
            for rank in range(G):
                part, sp = dev.render_stripes(cam, p, 4, rank, G)
                rows = [api.stripe_row_index(H, 4, rank, G, i) for i in range(part.shape[0])]
                film[rows] = part; rays += sp.rays
            assert np.array_equal(film.view(np.uint32), tile.view(np.uint32)) and rays == st.rays, G
        # sample batches / progressive passes 2 + 3 + 1 against one shot
        one, _ = dev.render_stripes(cam, p, 8, 0, 1)
        acc = np.zeros_like(one)
        for first, n in ((0, 2), (2, 3), (5, 1)):
            dev.render_stripes_accumulate(cam, p, 8, 0, 1, acc, first, n)
        assert np.array_equal(acc.view(np.uint32), one.view(np.uint32))
        acc = np.zeros_like(one)
        for s in range(spp):
            dev.render_stripes_accumulate(cam, p, 8, 0, 1, acc, s, 1)
        assert np.array_equal(acc.view(np.uint32), one.view(np.uint32))
        # adaptive with threshold 0 = uniform
        mean, count, _ = dev.render_adaptive(cam, p, api.Adaptive(2, 3, 0.0, 0.0))
        assert (count == spp).all()
        assert np.array_equal(mean.reshape(one.shape).view(np.uint32), one.view(np.uint32))
        # loopback multi-GPU session: G = 3 on one device equals G = 1 equals the tile -- once it has been given the parameters
        films = []
        for devices in ((0,), (0, 0, 0)):
            m = api.MultiScene(hs.flat_ptr, devices=devices, loopback=True)
            try:
                m.set_roulette(*params)
                sums, _, ms = m.render(cam, p, rows_per_block=8, want_u8=False)
                assert ms.rays == st.rays
            finally:
                m.close()
            films.append(sums)
        assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32))
        assert np.array_equal(films[0].view(np.uint32), tile.view(np.uint32))
    finally:
        dev.set_roulette()


def test_the_parameters_reach_the_kernels_and_the_setter_refuses_bad_ones(cornell):
    api, hs, dev = cornell
    cam = hs.camera(32, 32)
    p = api.default_params(32, 32, 4, seed=5, roulette=True)
    films = {}
    try:
        for params in ((3, 0.05), (0, 0.05), (3, 0.5), (1000, 0.05), (0, 1.0)):
            dev.set_roulette(*params)
            films[params] = dev.render_tile(cam, p)
        for bad in ((-1, 0.05), (3, 0.0), (3, 1.5), (3, float("nan"))):
            with pytest.raises(api.HrtError) as e:
                dev.set_roulette(*bad)
            assert e.value.status == api.HRT_ERR_INVALID
        again = dev.render_tile(cam, p)                     # a refused call left the parameters alone
        assert np.array_equal(again[0].view(np.uint32), films[(0, 1.0)][0].view(np.uint32))
    finally:
        dev.set_roulette()
    plain = dev.render_tile(cam, api.default_params(32, 32, 4, seed=5))
    rays = {k: v[1].rays for k, v in films.items()}
    assert rays[(0, 0.05)] < rays[(3, 0.05)] < plain[1].rays and rays[(3, 0.5)] != rays[(3, 0.05)]
    # never reached (max_depth 50 < 1000), and a floor of 1 (q = 1 everywhere): the default film and count, through the roulette kernels
    for off in ((1000, 0.05), (0, 1.0)):
        assert rays[off] == plain[1].rays and np.array_equal(films[off][0].view(np.uint32), plain[0].view(np.uint32)), off


def test_megakernel_and_stats_refuse_roulette(cornell):
    api, hs, dev = cornell
    for kw in (dict(megakernel=True), dict(stats=True), dict(stats=True, nee=True, stratified=True)):
        with pytest.raises(api.HrtError) as e:
            dev.render_tile(hs.camera(16, 16), api.default_params(16, 16, 1, roulette=True, **kw))
        assert e.value.status == api.HRT_ERR_UNSUPPORTED, kw
    dev.render_tile(hs.camera(16, 16), api.default_params(16, 16, 1, roulette=True, timing=True, progress=True, thin_lens=True))


def test_cli_roulette_and_checkpoints(built, assets, scenes_dir, tmp_path):
    import json
    from hobbyraytracer_amd import api
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    common = ["s.yaml", "--size", "48x32", "--spp", "4", "--seed", "2", "--no-progress"]

    def run(*extra):
        return subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=600)

    def rays(p):
        return json.loads([line for line in p.stdout.splitlines() if line.startswith("{")][-1])["rays"]
    p = run("--out", "plain.png", "--dump-linear", "plain.pfm", "--stats")
    assert p.returncode == 1, p.stderr             # Film::outputFilm's 1 = success (Q-12)
    rays_plain = rays(p)
    p = run("--roulette", "--out", "rr.png", "--dump-linear", "rr.pfm", "--stats")
    assert p.returncode == 1, p.stderr
    rays_rr = rays(p)
    p = run("--roulette-start", "3", "--roulette-floor", "0.05", "--out", "rr2.png", "--dump-linear", "rr2.pfm")    # the defaults, spelled out
    assert p.returncode == 1, p.stderr
    p = run("--roulette-start", "0", "--out", "rr0.png", "--dump-linear", "rr0.pfm", "--stats")
    assert p.returncode == 1, p.stderr
    rays_rr0 = rays(p)
    p = run("--roulette-floor", "0.5", "--out", "rrf.png", "--dump-linear", "rrf.pfm")
    assert p.returncode == 1, p.stderr
    pfm = {n: (tmp_path / f"{n}.pfm").read_bytes() for n in ("plain", "rr", "rr2", "rr0", "rrf")}
    assert pfm["rr"] == pfm["rr2"] and len({pfm["plain"], pfm["rr"], pfm["rr0"], pfm["rrf"]}) == 4
    assert rays_rr0 < rays_rr < rays_plain
    p = run("--roulette", "--nee", "--stratified", "--adaptive", "0.05", "--min-samples", "2", "--out", "ad.png")
    assert p.returncode == 1, p.stderr
    # a roulette checkpoint resumes only with the flag and the same two parameters; a plain one not with the flag
    p = run("--roulette", "--out", "a.png", "--progressive", "2", "--checkpoint", "rr.ck", "--max-passes", "1")
    assert p.returncode == 1, p.stderr
    for other in ((), ("--roulette-start", "2"), ("--roulette-floor", "0.1"), ("--roulette", "--stratified")):
        p = run(*other, "--out", "a.png", "--progressive", "2", "--checkpoint", "rr.ck", "--resume")
        assert p.returncode != 1 and "different render" in p.stderr, other
    p = run("--out", "b.png", "--progressive", "2", "--checkpoint", "plain.ck", "--max-passes", "1")
    assert p.returncode == 1, p.stderr
    p = run("--roulette", "--out", "b.png", "--progressive", "2", "--checkpoint", "plain.ck", "--resume")
    assert p.returncode != 1 and "different render" in p.stderr
    p = run("--roulette", "--out", "c.png", "--progressive", "2", "--checkpoint", "rr.ck", "--resume", "--dump-linear", "c.pfm")
    assert p.returncode == 1, p.stderr
    assert (tmp_path / "c.pfm").read_bytes() == pfm["rr"]                 # resumed = one shot, bit for bit


def test_off_is_off(built, tmp_path):
    """Without the flag the film and st.rays of cornell_box and teapot_scene are tests/golden/films.npz's, as before this flag existed --
    also on a scene whose roulette parameters have been set, and after a roulette render on it."""
    import importlib.util
    from hobbyraytracer_amd import api
    here = os.path.dirname(__file__)
    spec = importlib.util.spec_from_file_location("make_film_fixtures", os.path.join(here, "golden", "make_film_fixtures.py"))
    mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)
    mk.assets(str(tmp_path))
    want = np.load(os.path.join(here, "golden", "films.npz"))
    seen = 0
    for scene, W, H, spp in mk.CASES:
        if scene.split(".")[0] not in ("cornell_box", "teapot_scene"):
            continue
        seen += 1
        hs = api.HostScene(os.path.join(here, "golden", "scenes", scene), str(tmp_path))
        dev = api.DeviceScene(hs.flat_ptr, 0)
        try:
            cam = hs.camera(W, H)
            dev.set_roulette(0, 0.5)
            _, st_rr = dev.render_tile(cam, api.default_params(W, H, spp, seed=11, roulette=True))
            for qn, q in (("ref", api.QUIRKS_REFERENCE), ("fixed", api.QUIRKS_FIXED)):
                key = f"{scene.split('.')[0]}_{qn}"
                img, st = dev.render_tile(cam, api.default_params(W, H, spp, quirks=q, seed=11))
                b = want[key]
                same = (img.view(np.uint32) == b.view(np.uint32)) | (np.isnan(img) & np.isnan(b))
                assert same.all(), (key, int((~same).sum()))
                assert st.rays == int(want[key + "_rays"][0]), key
                assert qn != "ref" or st_rr.rays < st.rays
        finally:
            dev.close()
    assert seen == 2


SEGMENT_CASES = {"cornell_box": ("cornell_box.yaml", 256, 256, 64, dict(nee=True)), "teapot_scene": ("teapot_scene.yaml", 640, 640, 100, dict())}


def segment_ratio(api, dev, cam, W, H, spp, kw, seed):
    """-> (st.rays with the flag / without it, the count without it); default parameters"""
    _, a = dev.render_stripes(cam, api.default_params(W, H, spp, seed=seed, **kw), 8, 0, 1)
    _, b = dev.render_stripes(cam, api.default_params(W, H, spp, seed=seed, roulette=True, **kw), 8, 0, 1)
    return b.rays / a.rays, a.rays


@pytest.mark.parametrize("name", list(SEGMENT_CASES))
def test_roulette_traces_far_fewer_segments(built, assets_full, scenes_dir, name):
    """Bound: half the measured saving, ratio <= 1 - (1 - measured) / 2 (0.714 and 0.689), which must lie at least three seed-to-seed
    spreads above the measured ratio; the count without the flag is the one from before the flag, to the segment."""
    from hobbyraytracer_amd import api
    measured, spread = SEGMENTS_MEASURED[name]
    bound = 1.0 - (1.0 - measured) / 2.0
    assert bound >= measured + 3.0 * spread
    scene, W, H, spp, kw = SEGMENT_CASES[name]
    hs = api.HostScene(os.path.join(scenes_dir, scene), assets_full)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        ratio, rays0 = segment_ratio(api, dev, hs.camera(W, H), W, H, spp, kw, 0)
        _report(f"{name} {W}x{H} {spp} spp {sorted(kw)}: segments with roulette / without = {ratio:.4f} (measured {measured}, bound {bound:.4f}); without: {rays0}")
        assert rays0 == SEGMENTS_WITHOUT[name], (rays0, SEGMENTS_WITHOUT[name])
        assert ratio <= bound, (ratio, bound)
    finally:
        dev.close()
