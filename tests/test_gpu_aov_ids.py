"""Id mattes and position (hrt_render_aov_ids_*) on the GPU.

(a) At one sample rank 0 is the CPU oracle's first hit of the film's own camera ray, bit for bit: the object id is the primitive, the
    material id that primitive's material, the coverage 1, the position the hit's p; a miss is -1, coverage 1 and position 0; ranks 1 to
    3 are unused.  One sample's position v reaches the buffer as (+0 + v) / 1: v itself, except that -0 comes out as +0 (_acc).
(b) The table logic: a call over S samples equals tests/aov_ids_np.py's restatement of the header applied to the GPU's own S one-sample
    calls, bit for bit -- on a film some pixel of which sees more than eight objects and some pixel of which has a count tie that
    decides the report.
(c) Tiles, stripes of 1 to 4 ranks and the host and device-pointer forms give the same bits, with either sampler; the lens, the seed and
    the quirks change the output, the estimator's flags do not.
(d) The film does not notice the pass.  (e) Bad arguments are refused with the buffer untouched.  (f) The CLI's files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import aov_ids_np as ref
from tests import scene_helpers
from tests.test_gpu_stratified import _five_scenes

pytestmark = pytest.mark.gpu

W1, H1 = 24, 16          # parity film: one block of 256 threads and half of a second
GROUPS = ("position", "object_id", "object_coverage", "material_id", "material_coverage")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _acc(v, n=1):
    """what the position holds after one sample of value v of a call over n"""
    return (np.float32(0) + np.asarray(v, np.float32)) / np.float32(n)


def _with(api, p, **kw):
    q = api.Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _same(a, b):
    """two dicts of split_aov_ids hold the same bits"""
    return all(np.array_equal(_bits(a[g]), _bits(b[g])) for g in GROUPS)


def _raw(api, d):
    """a dict of split_aov_ids back as the raw buffer [h, w] of AOV_IDS_DTYPE"""
    out = np.zeros(d["object_id"].shape[:-1], api.AOV_IDS_DTYPE)
    out["position"][..., 0:3] = d["position"]
    for g in GROUPS[1:]:
        out[g] = d[g]
    return out


@pytest.fixture(scope="module")
def parity_scenes(built, assets, scenes_dir, tmp_path_factory):
    """name -> HostScene, the scenes of tests/test_gpu_aov.py's parity test: tests/test_gpu_stratified.py's five (material_zoo among
    them: textures, metal, glass, pbr), a random world with meshes, image textures and a medium, one object of every kind under a chain
    of three wrappers, and lights with looked-up emission"""
    from hobbyraytracer_amd import api
    out = dict(_five_scenes(assets, scenes_dir, tmp_path_factory.mktemp("five")))
    d = tmp_path_factory.mktemp("random_world")
    for seed in range(100, 200):
        path = scene_helpers.random_world(d, seed, False, meshes=True, images=True)
        text = open(path).read()
        if "constant_medium" in text and "type: mesh" in text:
            break
    else:
        raise AssertionError("no random world with a medium")
    out["random_world"] = api.HostScene(path, str(d))
    d = tmp_path_factory.mktemp("chain")
    out["wrapper_chain"] = api.HostScene(scene_helpers.wrapper_chain_scene(d, "YST"), str(d))
    d = tmp_path_factory.mktemp("textured_lights")
    out["textured_lights"] = api.HostScene(_textured_lights_scene(api, d), str(d))
    return out


def _textured_lights_scene(api, d):
    """Lights whose emission is looked up (an image albedo, a checkered albedo under a texture-valued strength, a bright image albedo)
    on a rect, a sphere and a rotated box over a floor."""
    api.write_image(str(d / "lamp.png"), np.random.default_rng(5).integers(0, 256, (5, 7, 3)).astype(np.uint8))
    (d / "lights.yaml").write_text(
        "film:\n    width: 32\n    height: 24\n    samples: 1\n    output: o.png\n"
        "camera:\n    position: [0, 1, 6]\n    look_at: [0, 1, 0]\n    up: [0, 1, 0]\n    fov: 45\n    aperture: 0.1\n"
        "    focal_distance: 6\n    background: [0.2, 0.3, 0.5]\n"
        "textures:\n  - name: img\n    type: image\n    path: lamp.png\n"
        "  - name: chk\n    type: checkered\n    even: [0.9, 0.7, 0.2]\n    odd: [0.1, 0.3, 0.6]\n"
        "materials:\n  - name: dim\n    type: diffuse_light\n    albedo: img\n    strength: 0.7\n"
        "  - name: varying\n    type: diffuse_light\n    albedo: chk\n    strength: img\n"
        "  - name: bright\n    type: diffuse_light\n    albedo: img\n    strength: 4\n"
        "  - name: floor\n    type: lambertian\n    albedo: [0.5, 0.5, 0.5]\n"
        "objects:\n"
        "  - type: xy_rect\n    x: [-2.4, -0.6]\n    y: [0.2, 1.8]\n    k: 0\n    material: dim\n"
        "  - type: sphere\n    center: [0.5, 1, 0]\n    radius: 0.8\n    material: varying\n"
        "  - type: box\n    center: [2, 1, 0]\n    dimensions: [1, 1.4, 1]\n    material: bright\n    transform:\n        rotate_y: 25\n"
        "  - type: xz_rect\n    x: [-4, 4]\n    z: [-4, 4]\n    k: -0.2\n    material: floor\n")
    return str(d / "lights.yaml")


def oracle_first_hits(api, orc, world, cam, p):
    """The oracle's first hit of its own camera ray of sample 0 of every pixel of the film (row-major): hit records [n]."""
    p1 = _with(api, p, max_depth=1)
    rays = np.array([orc.trace_path(world, cam, p1, pidx, 0, max_seg=1)[0][0] for pidx in range(p.width * p.height)], np.float32)
    o, d = np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:])
    return world.closest_hit(p, o, d, p.t_min, float("inf"), pixel0=0)


# ---- (a) ----
MATERIAL_KINDS = ("MAT_LAMBERTIAN", "MAT_METAL", "MAT_DIELECTRIC", "MAT_DIFFUSE_LIGHT", "MAT_ISOTROPIC", "MAT_PBR", "MAT_UVTEST")


@pytest.mark.parametrize("thin_lens", [False, True], ids=["pinhole", "thin_lens"])
@pytest.mark.parametrize("quirks", ["reference", "fixed"])
def test_one_sample_is_the_oracles_first_hit(parity_scenes, quirks, thin_lens):
    from hobbyraytracer_amd import api
    from oracle import oracle_py as orc
    q = api.QUIRKS_REFERENCE if quirks == "reference" else api.QUIRKS_FIXED
    n = W1 * H1
    seen = {}
    for name, hs in parity_scenes.items():
        cam = hs.camera(W1, H1)
        p = api.default_params(W1, H1, 1, quirks=q, seed=7, thin_lens=thin_lens)
        flat = hs.flat
        world = orc.World(hs.flat_ptr)
        dev = api.DeviceScene(hs.flat_ptr, 0)
        try:
            hits = oracle_first_hits(api, orc, world, cam, p)
            got = dev.render_aov_ids_tile(cam, p)
        finally:
            dev.close(); world.close()
        prim = hits["prim"].astype(np.int32)
        hit = prim >= 0
        prim_mat = np.array([flat.prims[i].material for i in range(flat.n_prims)] or [0], np.int32)
        prim_kind = np.array([flat.prims[i].kind for i in range(flat.n_prims)] or [0])
        want_obj = np.where(hit, prim, -1).astype(np.int32)
        want_mat = np.where(hit, prim_mat[np.where(hit, prim, 0)], -1).astype(np.int32)
        want_pos = np.where(hit[:, None], hits["p"], np.float32(0)).astype(np.float32)
        oid, ocov = got["object_id"].reshape(n, 4), got["object_coverage"].reshape(n, 4)
        mid, mcov = got["material_id"].reshape(n, 4), got["material_coverage"].reshape(n, 4)
        assert np.array_equal(oid[:, 0], want_obj), (name, "object id", np.argwhere(oid[:, 0] != want_obj)[:5])
        assert np.array_equal(mid[:, 0], want_mat), (name, "material id", np.argwhere(mid[:, 0] != want_mat)[:5])
        one = np.float32(1).view(np.uint32)
        for ids, cov in ((oid, ocov), (mid, mcov)):
            assert (_bits(cov[:, 0]) == one).all(), (name, "coverage of rank 0")
            assert (ids[:, 1:] == api.AOV_ID_UNUSED).all() and (_bits(cov[:, 1:]) == 0).all(), (name, "ranks 1 to 3")
        pos = got["position"].reshape(n, 3)
        bad = (_bits(pos) != _bits(_acc(want_pos))).any(axis=1)
        assert not bad.any(), (name, "position", int(bad.sum()), pos[bad][:3], want_pos[bad][:3])
        assert (_bits(pos[~hit]) == 0).all() and (oid[~hit, 0] == -1).all() and (mid[~hit, 0] == -1).all(), (name, "miss")
        seen["miss"] = seen.get("miss", 0) + int((~hit).sum())
        seen["medium"] = seen.get("medium", 0) + int((hit & (prim_kind[np.where(hit, prim, 0)] == api.PRIM_MEDIUM)).sum())
        for kind in MATERIAL_KINDS:
            mats = [i for i in range(flat.n_materials) if flat.materials[i].kind == getattr(api, kind)]
            seen[kind] = seen.get(kind, 0) + int(np.isin(mid[:, 0], mats).sum())
    print(seen)
    for what in MATERIAL_KINDS + ("miss", "medium"):
        assert seen.get(what, 0) > 0, (what, seen)


# ---- (b) ----
@pytest.fixture(scope="module")
def cornell(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "cornell_box.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


def _single_samples(api, dev, cam, p, stratified=False):
    """the GPU's own per-sample values: S calls with sample_first = s, sample_count = 1 -> object ids [S, h, w], material ids, positions"""
    obj, mat, pos = [], [], []
    for s in range(p.samples):
        one = api.split_aov_ids(dev.render_aov_ids_stripes(cam, p, 8, 0, 1, None, s, 1))
        assert (one["object_id"][..., 1:] == api.AOV_ID_UNUSED).all() and (one["object_coverage"][..., 0] == 1).all()
        assert (one["material_id"][..., 1:] == api.AOV_ID_UNUSED).all() and (one["material_coverage"][..., 0] == 1).all()
        obj.append(one["object_id"][..., 0].copy()); mat.append(one["material_id"][..., 0].copy()); pos.append(one["position"].copy())
    return np.array(obj), np.array(mat), np.array(pos)


def test_cornell_16_samples_is_the_restatement_of_its_single_samples(cornell):
    api, hs, dev = cornell
    W, H, S = 24, 16, 16
    cam, p = hs.camera(W, H), api.default_params(W, H, S, seed=3)
    got = dev.render_aov_ids_tile(cam, p)
    obj, mat, pos = _single_samples(api, dev, cam, p)
    want = ref.mattes(obj, mat, pos)
    assert (got["object_id"][..., 1] != api.AOV_ID_UNUSED).any()          # some pixel straddles an edge
    for g in GROUPS:
        assert np.array_equal(_bits(got[g]), _bits(want[g])), (g, np.argwhere(_bits(got[g]) != _bits(want[g]))[:5])
    # a sub-range of the samples starts from empty tables too, and divides by its own count
    part = api.split_aov_ids(dev.render_aov_ids_stripes(cam, p, 8, 0, 1, None, 5, 7))
    want = ref.mattes(obj[5:12], mat[5:12], pos[5:12])
    for g in GROUPS:
        assert np.array_equal(_bits(part[g]), _bits(want[g])), g


MANY_MESHES, MANY_SEED = 40, 1


def test_crowded_pixels_drop_late_ids_and_break_ties_by_id(built, tmp_path):
    from hobbyraytracer_amd import api
    hs = api.HostScene(scene_helpers.many_meshes_scene(tmp_path, MANY_MESHES, MANY_SEED), str(tmp_path))
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        W = H = 4
        S = 64
        cam, p = hs.camera(W, H), api.default_params(W, H, S, seed=9)
        got = dev.render_aov_ids_tile(cam, p)
        obj, mat, pos = _single_samples(api, dev, cam, p)
    finally:
        dev.close()
    # the film is chosen so that the two rules that only show in a crowd are exercised; asserted, so that the test cannot pass vacuously
    distinct = np.array([[len(set(obj[:, y, x].tolist())) for x in range(W)] for y in range(H)])
    print("distinct objects per pixel:\n", distinct)
    assert (distinct > ref.SLOTS).any(), distinct
    ties = 0
    for y in range(H):
        for x in range(W):
            order = sorted(ref.table(obj[:, y, x]), key=lambda s: (-s[1], s[0]))
            ties += any(order[k][1] == order[k + 1][1] for k in range(min(ref.RANKS, len(order) - 1)))     # ranks 0..3 against their successor
    assert ties > 0, "no pixel whose report depends on the order of equal counts"
    want = ref.mattes(obj, mat, pos)
    for g in GROUPS:
        assert np.array_equal(_bits(got[g]), _bits(want[g])), (g, np.argwhere(_bits(got[g]) != _bits(want[g]))[:5])
    dropped = np.float32(1) - api.matte(got["object_id"], got["object_coverage"], list(range(-1, hs.flat.n_prims)))
    assert (dropped[distinct > ref.RANKS] > 0).all()


# ---- (c) ----
@pytest.mark.parametrize("stratified", [False, True], ids=["philox", "stratified"])
def test_forms_agree_bit_for_bit(cornell, stratified):
    import torch
    api, hs, dev = cornell
    W, H, spp = 24, 16, 5
    cam = hs.camera(W, H)
    p = api.default_params(W, H, spp, seed=3, stratified=stratified)
    tile = dev.render_aov_ids_tile(cam, p)
    raw = _raw(api, tile)
    assert raw.shape == (H, W) and (tile["object_id"][..., 0] >= 0).any()
    # tiles: four rectangles of unequal size
    film = np.zeros((H, W), api.AOV_IDS_DTYPE)
    for x0, y0, w, h in ((0, 0, 9, 5), (9, 0, 15, 5), (0, 5, 14, 11), (14, 5, 10, 11)):
        film[y0:y0 + h, x0:x0 + w] = _raw(api, dev.render_aov_ids_tile(cam, p, (x0, y0, w, h)))
    assert film.tobytes() == raw.tobytes()
    # stripes of 1, 2, 3 and 4 ranks, host form (into a buffer that was never cleared) and device-pointer form
    for G in (1, 2, 3, 4):
        film = np.zeros((H, W), api.AOV_IDS_DTYPE)
        dfilm = np.zeros((H, W), api.AOV_IDS_DTYPE)
        for rank in range(G):
            rows = api.stripe_rows(H, 4, rank, G)
            buf = np.frombuffer(bytes([0xA5]) * (rows * W * 80), api.AOV_IDS_DTYPE).reshape(rows, W).copy()
            part = dev.render_aov_ids_stripes(cam, p, 4, rank, G, buf)
            assert part is buf
            index = [api.stripe_row_index(H, 4, rank, G, i) for i in range(rows)]
            film[index] = part
            t = torch.full((rows * W * 20,), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            dev.render_aov_ids_stripes_device(cam, p, 4, rank, G, t.data_ptr())
            torch.cuda.synchronize()
            dfilm[index] = t.cpu().numpy().view(api.AOV_IDS_DTYPE).reshape(rows, W)
        assert film.tobytes() == raw.tobytes(), G
        assert dfilm.tobytes() == raw.tobytes(), G
    # the device-pointer form with a sample range, against the host form
    t = torch.zeros((H * W * 20,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dev.render_aov_ids_stripes_device(cam, p, 8, 0, 1, t.data_ptr(), 1, 3)
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == dev.render_aov_ids_stripes(cam, p, 8, 0, 1, None, 1, 3).tobytes() != raw.tobytes()


def test_only_the_lens_the_sampler_the_seed_and_the_quirks_matter(cornell, parity_scenes):
    api, hs, dev = cornell
    W, H, spp = 24, 16, 3
    cam = hs.camera(W, H)
    base = dev.render_aov_ids_tile(cam, api.default_params(W, H, spp, seed=5))
    for kw in (dict(nee=True), dict(nee_env=True), dict(nee_emitters=True), dict(nee_lobes=True), dict(roulette=True), dict(timing=True),
               dict(progress=True), dict(nee_lobes=True, nee_env=True, nee_emitters=True, roulette=True, timing=True, progress=True)):
        assert _same(dev.render_aov_ids_tile(cam, api.default_params(W, H, spp, seed=5, **kw)), base), kw
    for flags in (api.FLAG_NEE_ENV, api.FLAG_MEGAKERNEL | api.FLAG_NEE, api.FLAG_STATS | api.FLAG_ROULETTE):     # no other flag is read
        p = api.default_params(W, H, spp, seed=5)
        p.flags = flags
        assert _same(dev.render_aov_ids_tile(cam, p), base), flags
    for kw in (dict(seed=6), dict(seed=5, thin_lens=True), dict(seed=5, stratified=True)):
        assert not _same(dev.render_aov_ids_tile(cam, api.default_params(W, H, spp, **kw)), base), kw
    # the quirks: the teapot's triangles are intersected along another axis (Q-4), so the hit points' bits move
    ths = parity_scenes["teapot_scene"]
    tdev = api.DeviceScene(ths.flat_ptr, 0)
    try:
        tcam = ths.camera(W, H)
        a = tdev.render_aov_ids_tile(tcam, api.default_params(W, H, spp, seed=5, quirks=api.QUIRKS_REFERENCE))
        b = tdev.render_aov_ids_tile(tcam, api.default_params(W, H, spp, seed=5, quirks=api.QUIRKS_FIXED))
    finally:
        tdev.close()
    assert not _same(a, b)


# ---- (d) ----
def test_the_film_is_unchanged(cornell, tmp_path):
    import importlib.util
    api, hs, dev = cornell
    W, H, spp = 24, 16, 3
    cam = hs.camera(W, H)
    for kw in (dict(), dict(nee=True, stratified=True, roulette=True)):
        p = api.default_params(W, H, spp, seed=5, **kw)
        before, st0 = dev.render_tile(cam, p)
        dev.render_aov_ids_tile(cam, p)
        after, st1 = dev.render_tile(cam, p)
        assert np.array_equal(_bits(before), _bits(after)) and st0.rays == st1.rays and st0.samples == st1.samples == W * H * spp, kw
    # the committed films of cornell_box and teapot_scene reproduce, to the segment count, with an ids call in front of each render
    here = os.path.dirname(__file__)
    spec = importlib.util.spec_from_file_location("make_film_fixtures", os.path.join(here, "golden", "make_film_fixtures.py"))
    mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)
    mk.assets(str(tmp_path))
    want = np.load(os.path.join(here, "golden", "films.npz"))
    seen = 0
    for scene, fw, fh, fspp in mk.CASES:
        if scene.split(".")[0] not in ("cornell_box", "teapot_scene"):
            continue
        seen += 1
        ghs = api.HostScene(os.path.join(here, "golden", "scenes", scene), str(tmp_path))
        gdev = api.DeviceScene(ghs.flat_ptr, 0)
        try:
            gcam = ghs.camera(fw, fh)
            for qn, q in (("ref", api.QUIRKS_REFERENCE), ("fixed", api.QUIRKS_FIXED)):
                key = f"{scene.split('.')[0]}_{qn}"
                gp = api.default_params(fw, fh, fspp, quirks=q, seed=11)
                gdev.render_aov_ids_tile(gcam, _with(api, gp, samples=min(fspp, 2)))
                img, st = gdev.render_tile(gcam, gp)
                b = want[key]
                same = (img.view(np.uint32) == b.view(np.uint32)) | (np.isnan(img) & np.isnan(b))
                assert same.all(), (key, int((~same).sum()))
                assert st.rays == int(want[key + "_rays"][0]), key
        finally:
            gdev.close()
    assert seen == 2


# ---- (e) ----
def test_bad_arguments_are_refused_and_leave_the_buffer_alone(cornell):
    import torch
    api, hs, dev = cornell
    W, H, spp = 16, 12, 6
    cam, p = hs.camera(W, H), api.default_params(W, H, spp)
    hip, h = api._hip, dev._h
    out = np.full((H, W, 20), 7.0, np.float32)
    ptr = C.c_void_p(out.ctypes.data)
    t = torch.full((H, W, 20), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dptr = C.c_void_p(t.data_ptr())
    cb, pb = C.byref(cam), C.byref(p)
    full = api.Rect(0, 0, W, H)
    calls = {
        "tile: NULL camera": lambda: hip.hrt_render_aov_ids_tile(h, None, pb, full, ptr),
        "tile: NULL params": lambda: hip.hrt_render_aov_ids_tile(h, cb, None, full, ptr),
        "tile: NULL buffer": lambda: hip.hrt_render_aov_ids_tile(h, cb, pb, full, None),
        "tile: empty": lambda: hip.hrt_render_aov_ids_tile(h, cb, pb, api.Rect(0, 0, 0, H), ptr),
        "tile: empty rows": lambda: hip.hrt_render_aov_ids_tile(h, cb, pb, api.Rect(0, 0, W, 0), ptr),
        "tile: negative origin": lambda: hip.hrt_render_aov_ids_tile(h, cb, pb, api.Rect(-1, 0, 4, 4), ptr),
        "tile: past the right edge": lambda: hip.hrt_render_aov_ids_tile(h, cb, pb, api.Rect(W - 3, 0, 4, 4), ptr),
        "tile: past the bottom": lambda: hip.hrt_render_aov_ids_tile(h, cb, pb, api.Rect(0, H - 3, 4, 4), ptr),
        "tile: samples 0": lambda: hip.hrt_render_aov_ids_tile(h, cb, C.byref(_with(api, p, samples=0)), full, ptr),
        "stripes: NULL camera": lambda: hip.hrt_render_aov_ids_stripes(h, None, pb, 4, 0, 1, ptr, 0, -1),
        "stripes: NULL params": lambda: hip.hrt_render_aov_ids_stripes(h, cb, None, 4, 0, 1, ptr, 0, -1),
        "stripes: NULL buffer": lambda: hip.hrt_render_aov_ids_stripes(h, cb, pb, 4, 0, 1, None, 0, -1),
        "stripes: sample_count 0": lambda: hip.hrt_render_aov_ids_stripes(h, cb, pb, 4, 0, 1, ptr, 0, 0),
        "stripes: range past samples": lambda: hip.hrt_render_aov_ids_stripes(h, cb, pb, 4, 0, 1, ptr, 2, spp - 1),
        "stripes: first == samples": lambda: hip.hrt_render_aov_ids_stripes(h, cb, pb, 4, 0, 1, ptr, spp, -1),
        "stripes: negative first": lambda: hip.hrt_render_aov_ids_stripes(h, cb, pb, 4, 0, 1, ptr, -1, 2),
        "stripes: rank == n_ranks": lambda: hip.hrt_render_aov_ids_stripes(h, cb, pb, 4, 2, 2, ptr, 0, -1),
        "stripes: rows_per_block 0": lambda: hip.hrt_render_aov_ids_stripes(h, cb, pb, 0, 0, 1, ptr, 0, -1),
        "device: NULL camera": lambda: hip.hrt_render_aov_ids_stripes_device(h, None, pb, 4, 0, 1, dptr, 0, -1, None),
        "device: NULL params": lambda: hip.hrt_render_aov_ids_stripes_device(h, cb, None, 4, 0, 1, dptr, 0, -1, None),
        "device: NULL buffer": lambda: hip.hrt_render_aov_ids_stripes_device(h, cb, pb, 4, 0, 1, None, 0, -1, None),
        "device: sample_count 0": lambda: hip.hrt_render_aov_ids_stripes_device(h, cb, pb, 4, 0, 1, dptr, 0, 0, None),
        "device: range past samples": lambda: hip.hrt_render_aov_ids_stripes_device(h, cb, pb, 4, 0, 1, dptr, spp - 1, 2, None),
        "device: rank == n_ranks": lambda: hip.hrt_render_aov_ids_stripes_device(h, cb, pb, 4, 1, 1, dptr, 0, -1, None),
        # (refused before anything is launched: the kernel's 16-byte stores never see the pointer)
        "device: buffer not 16-byte aligned": lambda: hip.hrt_render_aov_ids_stripes_device(h, cb, pb, 4, 0, 1, C.c_void_p(t.data_ptr() + 4), 0, -1, None),
        "device: buffer 8-byte aligned": lambda: hip.hrt_render_aov_ids_stripes_device(h, cb, pb, 4, 0, 1, C.c_void_p(t.data_ptr() + 8), 1, 2, None),
    }
    for what, call in calls.items():
        assert call() == api.HRT_ERR_INVALID, what
        assert hip.hrt_last_error(), what
        assert (out == 7.0).all(), what
    torch.cuda.synchronize()
    assert bool((t == 7.0).all())
    with pytest.raises(api.HrtError) as e:
        dev.render_aov_ids_tile(cam, p, (0, 0, W + 1, H))
    assert e.value.status == api.HRT_ERR_INVALID
    good = dev.render_aov_ids_stripes(cam, p, 4, 0, 1)               # and a good call still works, on both kinds of buffer
    dev.render_aov_ids_stripes_device(cam, p, 4, 0, 1, t.data_ptr())
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == good.tobytes() and (good["object_coverage"][..., 0] > 0).all()


# ---- (f) ----
def test_cli_aov_ids(cornell, tmp_path, scenes_dir):
    import json
    api, hs, dev = cornell
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    W, H = 24, 16
    common = ["s.yaml", "--size", f"{W}x{H}", "--spp", "4", "--seed", "2", "--no-progress"]

    def run(*extra):
        return subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    flat = hs.flat
    wanted_obj, wanted_mat = [0, flat.n_prims - 1], [1]
    r = run("--aov", "p", "--aov-spp", "3", "--aov-ids", "--matte", "object:" + ",".join(map(str, wanted_obj)), "mo.pfm",
            "--matte", "material:1", "mm.pfm", "--matte", "object:-1", "miss.pfm", "--dump-linear", "with.pfm", "--out", "a.png", "--stats")
    assert r.returncode == 1, r.stdout + r.stderr            # Film::outputFilm's 1 = success (Q-12)
    js = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert js["aov_spp"] == 3 and js["aov_ids_s"] > 0 and js["aov_s"] > 0 and js["samples"] == W * H * 4
    want = dev.render_aov_ids_tile(hs.camera(W, H), api.default_params(W, H, 3, seed=2))
    assert np.array_equal(_bits(api.read_pfm(str(tmp_path / "p.position.pfm"))), _bits(want["position"]))
    for kind in ("object", "material"):
        for k in range(4):
            img = api.read_pfm(str(tmp_path / f"p.{kind}{k}.pfm"))
            assert img.shape == (H, W, 3)
            assert np.array_equal(img[..., 0], want[kind + "_id"][..., k].astype(np.float32)), (kind, k)
            assert np.array_equal(_bits(img[..., 1]), _bits(want[kind + "_coverage"][..., k])) and (_bits(img[..., 2]) == 0).all(), (kind, k)
    assert (tmp_path / "p.albedo.pfm").exists()                # --aov's own files are still written
    # the mattes: api.matte of the buffers, in all three channels
    for name, kind, ids in (("mo.pfm", "object", wanted_obj), ("mm.pfm", "material", wanted_mat), ("miss.pfm", "object", [-1])):
        m = api.matte(want[kind + "_id"], want[kind + "_coverage"], ids)
        assert np.array_equal(_bits(api.read_pfm(str(tmp_path / name))), _bits(np.repeat(m[..., None], 3, axis=2))), name
    assert api.matte(want["material_id"], want["material_coverage"], wanted_mat).max() > 0
    # the manifest lists every prim and every material, with the names the scene file gave
    lines = (tmp_path / "p.ids.txt").read_text().splitlines()
    objects = [ln.split() for ln in lines if ln.startswith("object ")]
    materials = [ln.split() for ln in lines if ln.startswith("material ")]
    assert [int(o[1]) for o in objects] == list(range(flat.n_prims))
    assert [int(o[4]) for o in objects] == [flat.prims[i].material for i in range(flat.n_prims)]
    assert [int(m[1]) for m in materials] == list(range(flat.n_materials))
    text = open(os.path.join(scenes_dir, "cornell_box.yaml")).read()
    named = [m[3] for m in materials if len(m) > 3]
    assert named and all(f"name: {n}" in text for n in named), materials
    # --matte alone implies --aov-ids; without the new flags nothing new is written and the film is the same
    r = run("--aov", "q", "--aov-spp", "3", "--matte", "material:1", "q.pfm", "--out", "q.png")
    assert r.returncode == 1, r.stderr
    assert (tmp_path / "q.pfm").read_bytes() == (tmp_path / "mm.pfm").read_bytes() and (tmp_path / "q.ids.txt").exists()
    r = run("--aov", "n", "--aov-spp", "3", "--dump-linear", "without.pfm", "--out", "b.png", "--stats")
    assert r.returncode == 1, r.stderr
    assert "aov_ids_s" not in r.stdout
    assert not any((tmp_path / f"n.{x}").exists() for x in ("position.pfm", "object0.pfm", "material0.pfm", "ids.txt"))
    assert (tmp_path / "n.albedo.pfm").read_bytes() == (tmp_path / "p.albedo.pfm").read_bytes()
    assert (tmp_path / "without.pfm").read_bytes() == (tmp_path / "with.pfm").read_bytes()
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes()
    r = run("--aov-ids", "--out", "u.png")
    assert r.returncode == 2 and "--aov" in r.stderr, (r.returncode, r.stderr)
