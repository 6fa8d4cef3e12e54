"""Feature buffers (hrt_render_aov_*) on the GPU: at one sample every buffer is the CPU oracle's first hit of the film's
own camera ray, bit for bit (depth: 4 ulp); tiles, stripes, sample batches and the host and device-pointer forms give the same bits, and
the buffer is the plain fp32 mean of the per-sample values; the pass knows the lens, the sampler, the seed and the quirks and nothing else,
and leaves the film's render alone; bad arguments are refused with the output untouched; and the CLI's --aov writes the same buffers
whatever else the render is asked to do.

One sample's value v reaches the buffer as (+0 + v) / 1 (the accumulation rule of include/hrt.h): that is v itself, bit for bit, except
that a -0 comes out as +0.  The expected values below go through the same two operations (_acc)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import scene_helpers
from tests.test_gpu_stratified import _five_scenes

pytestmark = pytest.mark.gpu

W1, H1 = 32, 24          # parity film: two blocks of 256 threads and a part of a third


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _acc(v, n=1):
    """what a buffer holds after one sample of value v of params.samples = n"""
    return (np.float32(0) + np.asarray(v, np.float32)) / np.float32(n)


def _clamp01(c):
    """each channel to [0, 1], NaN -> 0"""
    c = np.asarray(c, np.float32)
    return np.where(np.isnan(c), np.float32(0), np.clip(c, np.float32(0), np.float32(1))).astype(np.float32)


def _with(api, p, **kw):
    q = api.Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


@pytest.fixture(scope="module")
def parity_scenes(built, assets, scenes_dir, tmp_path_factory):
    """name -> HostScene: tests/test_gpu_stratified.py's five (material_zoo among them: textures, metal, glass, pbr), a random world with
    meshes, image textures and a medium, one object of every kind under a chain of three wrappers, and lights with looked-up emission"""
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
    """Lights whose emission is looked up: an image albedo (strength below 1, so most values pass the clamp unchanged), a checkered
    albedo under a texture-valued strength, and an image albedo bright enough to be clamped.  No scene of the project's has one in view."""
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


def camera_rays(orc, world, cam, p):
    """the film's camera ray of sample 0 of every pixel, from the oracle's path tracer: (o [n, 3], d [n, 3])"""
    from hobbyraytracer_amd import api
    p1 = _with(api, p, max_depth=1)
    rays = np.array([orc.trace_path(world, cam, p1, pidx, 0, max_seg=1)[0][0] for pidx in range(p.width * p.height)], np.float32)
    return np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:])


def expected_first_hits(api, orc, hs, world, cam, p):
    """The oracle's side of the parity test for one scene: per pixel of the film (row-major) alpha, normal, depth (float64) and, per
    category of the issue, a mask and the expected albedo."""
    flat = hs.flat
    o, d = camera_rays(orc, world, cam, p)
    hits = world.closest_hit(p, o, d, p.t_min, float("inf"), pixel0=0)
    _, att, flag, _ = world.scatter(p, o, d, pixel0=0)
    prim = hits["prim"]
    hit = prim >= 0
    safe = np.where(hit, prim, 0)
    prim_kind = np.array([flat.prims[i].kind for i in range(flat.n_prims)] or [0])[safe]
    prim_mat = np.array([flat.prims[i].material for i in range(flat.n_prims)] or [0])[safe]
    mats = [flat.materials[i] for i in range(flat.n_materials)]

    def const(m):
        """the material's albedo when it is a constant, else None"""
        if m.albedo.tex < 0:
            return np.array(list(m.albedo.c), np.float32)
        t = flat.textures[m.albedo.tex]
        return np.array(list(t.c), np.float32) if t.kind == api.TEX_SOLID else None
    mat_kind = np.array([m.kind for m in mats])[prim_mat]
    medium = hit & (prim_kind == api.PRIM_MEDIUM)
    normal = np.where((hit & ~medium)[:, None], hits["normal"], np.float32(0)).astype(np.float32)
    depth = np.where(hit, hits["t"].astype(np.float64) * np.sqrt((d.astype(np.float64) ** 2).sum(axis=1)), 0.0)
    cats = {}
    for name, kind in (("lambertian", api.MAT_LAMBERTIAN), ("metal", api.MAT_METAL), ("isotropic", api.MAT_ISOTROPIC), ("uv_test", api.MAT_UVTEST)):
        cats[name] = (hit & (flag == 1) & (mat_kind == kind), att)
    cats["dielectric"] = (hit & (mat_kind == api.MAT_DIELECTRIC), np.ones_like(att))
    # a PBR's attenuation is its albedo whichever lobe its mix chooses (oracle.cpp PBR::scatter): the oracle's own lookup of the albedo,
    # so a looked-up albedo would be compared as well -- the scene loader reads a pbr's albedo as a constant only, none can be built here
    cats["pbr_scattered"] = (hit & (flag == 1) & (mat_kind == api.MAT_PBR), att)
    # what a light emits, from the oracle's one-segment film (max_depth 1: the emission at a light, nothing after it): its own
    # lookup of emit and strength, textures included
    emitted, _ = world.render_tile(cam, _with(api, p, max_depth=1))
    emitted = _clamp01(emitted.reshape(-1, 3))
    cats["light_emission"] = (hit & (mat_kind == api.MAT_DIFFUSE_LIGHT), emitted)
    table = np.zeros_like(att)
    light, pbr, looked_up = np.zeros_like(hit), np.zeros_like(hit), np.zeros_like(hit)
    for i, m in enumerate(mats):
        c = const(m)
        here = hit & (prim_mat == i)
        if m.kind == api.MAT_DIFFUSE_LIGHT and (c is None or m.s0.tex >= 0):
            looked_up |= here
        elif m.kind == api.MAT_DIFFUSE_LIGHT:
            table[here] = _clamp01(c * np.float32(m.s0.c)); light |= here
        elif m.kind == api.MAT_PBR:
            assert c is not None, "a pbr with a looked-up albedo: compare it in a category of its own"
            assert np.array_equal(c, _clamp01(c))         # (so the clamped and the un-clamped constant are one value)
            table[here] = c; pbr |= here
    cats["solid_light"] = (light, table)
    cats["pbr"] = (pbr, table)
    cats["textured_light"] = (looked_up, emitted)
    return {"hit": hit, "medium": medium, "normal": normal, "depth": depth, "cats": cats}


def check_parity(name, want, aov, film_depth1, seen):
    """one scene's buffers against expected_first_hits; counts the pixels of every category in `seen`"""
    n = want["hit"].size
    albedo, alpha, normal, depth = aov["albedo"].reshape(n, 3), aov["alpha"].reshape(n), aov["normal"].reshape(n, 3), aov["depth"].reshape(n)
    hit, miss = want["hit"], ~want["hit"]
    assert np.array_equal(_bits(alpha), _bits(hit.astype(np.float32))), (name, "alpha", np.argwhere(alpha != hit)[:5])
    assert np.array_equal(_bits(normal), _bits(_acc(want["normal"]))), (name, "normal", np.argwhere(_bits(normal) != _bits(_acc(want["normal"])))[:5])
    exact = want["depth"]
    fin = np.isfinite(exact)
    ulp = np.spacing(np.abs(exact[fin]).astype(np.float32)).astype(np.float64)
    err = np.abs(depth[fin].astype(np.float64) - exact[fin]) / ulp
    print(f"{name}: depth error max {err.max() if err.size else 0:.3f} ulp over {int(fin.sum())} pixels")
    assert (err <= 4.0).all(), (name, "depth", float(err.max()))
    with np.errstate(over="ignore", invalid="ignore"):
        assert np.array_equal(_bits(depth[~fin]), _bits(_acc(exact[~fin].astype(np.float32)))), (name, "non-finite depth")
    assert (_bits(depth[miss]) == 0).all() and (_bits(normal[miss]) == 0).all(), (name, "miss")
    for cat, (mask, value) in want["cats"].items():
        seen[cat] = seen.get(cat, 0) + int(mask.sum())
        bad = _bits(albedo[mask]) != _bits(_acc(value[mask]))
        assert not bad.any(), (name, cat, int(bad.sum()), albedo[mask][bad.any(axis=1)][:3], value[mask][bad.any(axis=1)][:3])
    seen["miss"] = seen.get("miss", 0) + int(miss.sum())
    seen["medium"] = seen.get("medium", 0) + int(want["medium"].sum())
    sky = _clamp01(film_depth1.reshape(n, 3)[miss])          # the miss branch's own value: a 1-sample, max_depth 1 film
    assert np.array_equal(_bits(albedo[miss]), _bits(_acc(sky))), (name, "background")


CATEGORIES = ("lambertian", "metal", "isotropic", "uv_test", "dielectric", "solid_light", "pbr", "pbr_scattered", "light_emission", "textured_light",
              "miss", "medium")


@pytest.mark.parametrize("thin_lens", [False, True], ids=["pinhole", "thin_lens"])
@pytest.mark.parametrize("quirks", ["reference", "fixed"])
def test_one_sample_is_the_oracles_first_hit(parity_scenes, quirks, thin_lens):
    from hobbyraytracer_amd import api
    from oracle import oracle_py as orc
    q = api.QUIRKS_REFERENCE if quirks == "reference" else api.QUIRKS_FIXED
    seen = {}
    for name, hs in parity_scenes.items():
        cam = hs.camera(W1, H1)
        p = api.default_params(W1, H1, 1, quirks=q, seed=7, thin_lens=thin_lens)
        world = orc.World(hs.flat_ptr)
        dev = api.DeviceScene(hs.flat_ptr, 0)
        try:
            want = expected_first_hits(api, orc, hs, world, cam, p)
            aov = dev.render_aov_tile(cam, p)
            film, _ = dev.render_tile(cam, _with(api, p, max_depth=1))
            check_parity(name, want, aov, film, seen)
        finally:
            dev.close(); world.close()
    print(seen)
    for cat in CATEGORIES:
        assert seen.get(cat, 0) > 0, (cat, seen)


def test_stratified_one_sample_agrees_with_its_own_film_on_misses_and_lights(parity_scenes):
    """The oracle's path tracer does not know the stratified sampler, so what is stated is what can be stated exactly: the stratified
    buffers differ from the default ones, and against a stratified 1-sample, max_depth 1 film (the background on a miss, the emission
    on a light, 0 elsewhere) albedo is the clamped film on every miss and on every pixel whose film is not 0."""
    from hobbyraytracer_amd import api
    misses = lights = 0
    for name in ("cornell_box", "mixed_lights", "teapot_scene"):
        hs = parity_scenes[name]
        cam = hs.camera(W1, H1)
        dev = api.DeviceScene(hs.flat_ptr, 0)
        try:
            p = api.default_params(W1, H1, 1, seed=7, stratified=True)
            aov = dev.render_aov_tile(cam, p)
            plain = dev.render_aov_tile(cam, api.default_params(W1, H1, 1, seed=7))
            film, _ = dev.render_tile(cam, _with(api, p, max_depth=1))
        finally:
            dev.close()
        assert not np.array_equal(_bits(aov["depth"]), _bits(plain["depth"])), name
        miss = aov["alpha"] == 0
        assert set(np.unique(aov["alpha"])) <= {0.0, 1.0}
        lit = ~miss & (film != 0).any(axis=2)
        assert np.array_equal(_bits(aov["albedo"][miss]), _bits(_acc(_clamp01(film[miss])))), name
        assert np.array_equal(_bits(aov["albedo"][lit]), _bits(_acc(_clamp01(film[lit])))), name
        assert (_bits(aov["normal"][miss]) == 0).all() and (_bits(aov["depth"][miss]) == 0).all()
        misses += int(miss.sum()); lights += int(lit.sum())
    assert misses > 0 and lights > 0, (misses, lights)


@pytest.fixture(scope="module")
def cornell(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "cornell_box.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


def _raw(aov):
    return np.concatenate([aov["albedo"], aov["alpha"][..., None], aov["normal"], aov["depth"][..., None]], axis=-1)


@pytest.mark.parametrize("stratified", [False, True], ids=["philox", "stratified"])
def test_aov_forms_agree_bit_for_bit(cornell, stratified):
    import torch
    api, hs, dev = cornell
    W, H, spp = 48, 40, 6
    cam = hs.camera(W, H)
    p = api.default_params(W, H, spp, seed=3, stratified=stratified)
    tile = _raw(dev.render_aov_tile(cam, p))
    assert tile.shape == (H, W, 8) and 0 < tile[..., 3].mean() <= 1
    # tiles: four rectangles of unequal size
    film = np.full_like(tile, np.nan)
    for x0, y0, w, h in ((0, 0, 17, 9), (17, 0, 31, 9), (0, 9, 30, 31), (30, 9, 18, 31)):
        film[y0:y0 + h, x0:x0 + w] = _raw(dev.render_aov_tile(cam, p, (x0, y0, w, h)))
    assert np.array_equal(_bits(film), _bits(tile))
    # stripes of 1, 2, 3 and 4 ranks
    for G in (1, 2, 3, 4):
        film = np.full_like(tile, np.nan)
        for rank in range(G):
            part = dev.render_aov_stripes(cam, p, 4, rank, G)
            film[[api.stripe_row_index(H, 4, rank, G, i) for i in range(part.shape[0])]] = part
        assert np.array_equal(_bits(film), _bits(tile)), G
    # sample batches 2 + 3 + 1 and 1 x 6 against one shot, host form (from a buffer that was never cleared) ...
    for batches in (((0, 2), (2, 3), (5, 1)), tuple((s, 1) for s in range(spp))):
        acc = np.full((H, W, 8), np.nan, np.float32)
        for first, n in batches:
            assert dev.render_aov_stripes(cam, p, 8, 0, 1, acc, first, n) is acc
        assert np.array_equal(_bits(acc), _bits(tile)), batches
        # ... and the device-pointer form, on a torch tensor
        t = torch.full((H, W, 8), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for first, n in batches:
            dev.render_aov_stripes_device(cam, p, 8, 0, 1, t.data_ptr(), first, n)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(tile)), batches
    t = torch.full((H, W, 8), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dev.render_aov_stripes_device(cam, p, 8, 0, 1, t.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(tile))
    # the mean rule: the per-sample values (a range that does not reach params.samples is not divided), summed in ascending order in
    # fp32 from +0 and divided once
    longer = _with(api, p, samples=spp + 1)
    total = np.zeros((H, W, 8), np.float32)
    for s in range(spp):
        one = dev.render_aov_stripes(cam, longer, 8, 0, 1, np.zeros((H, W, 8), np.float32), s, 1)
        total = total + one
    assert np.array_equal(_bits(total / np.float32(spp)), _bits(tile))
    assert not np.array_equal(_bits(one), _bits(tile))


def test_only_the_lens_the_sampler_the_seed_and_the_quirks_matter(cornell, built, tmp_path):
    import importlib.util
    api, hs, dev = cornell
    W, H, spp = 40, 24, 3
    cam = hs.camera(W, H)
    base = _raw(dev.render_aov_tile(cam, api.default_params(W, H, spp, seed=5)))
    for kw in (dict(nee=True), dict(nee_env=True), dict(nee_emitters=True), dict(nee_lobes=True), dict(roulette=True), dict(timing=True),
               dict(progress=True), dict(nee_lobes=True, nee_env=True, nee_emitters=True, roulette=True, timing=True, progress=True)):
        assert np.array_equal(_bits(_raw(dev.render_aov_tile(cam, api.default_params(W, H, spp, seed=5, **kw)))), _bits(base)), kw
    # (flag combinations the film's render refuses are not refused here: no other flag is read)
    for flags in (api.FLAG_NEE_ENV, api.FLAG_MEGAKERNEL | api.FLAG_NEE, api.FLAG_STATS | api.FLAG_ROULETTE):
        p = api.default_params(W, H, spp, seed=5)
        p.flags = flags
        assert np.array_equal(_bits(_raw(dev.render_aov_tile(cam, p))), _bits(base)), flags
    for kw in (dict(seed=6), dict(seed=5, thin_lens=True), dict(seed=5, stratified=True)):
        assert not np.array_equal(_bits(_raw(dev.render_aov_tile(cam, api.default_params(W, H, spp, **kw)))), _bits(base)), kw
    # the film's render before and after a feature-buffer call on the same scene
    for kw in (dict(), dict(nee=True, stratified=True, roulette=True)):
        p = api.default_params(W, H, spp, seed=5, **kw)
        before, st0 = dev.render_tile(cam, p)
        dev.render_aov_tile(cam, p)
        after, st1 = dev.render_tile(cam, p)
        assert np.array_equal(_bits(before), _bits(after)) and st0.rays == st1.rays and st0.samples == st1.samples == W * H * spp, kw
    # the committed films of cornell_box and teapot_scene still reproduce, with a feature-buffer call in front of each render
    # (tests/test_gpu_roulette.py::test_off_is_off's loop)
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
                gdev.render_aov_tile(gcam, _with(api, gp, samples=min(fspp, 2)))
                img, st = gdev.render_tile(gcam, gp)
                b = want[key]
                same = (img.view(np.uint32) == b.view(np.uint32)) | (np.isnan(img) & np.isnan(b))
                assert same.all(), (key, int((~same).sum()))
                assert st.rays == int(want[key + "_rays"][0]), key
        finally:
            gdev.close()
    assert seen == 2


def test_bad_arguments_are_refused_and_leave_the_buffer_alone(cornell):
    import torch
    api, hs, dev = cornell
    W, H, spp = 16, 12, 6
    cam, p = hs.camera(W, H), api.default_params(W, H, spp)
    hip, h = api._hip, dev._h
    out = np.full((H, W, 8), 7.0, np.float32)
    ptr = out.ctypes.data_as(C.POINTER(C.c_float))
    t = torch.full((H, W, 8), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dptr = C.c_void_p(t.data_ptr())
    cb, pb = C.byref(cam), C.byref(p)
    full = api.Rect(0, 0, W, H)
    calls = {
        "tile: NULL camera": lambda: hip.hrt_render_aov_tile(h, None, pb, full, ptr),
        "tile: NULL params": lambda: hip.hrt_render_aov_tile(h, cb, None, full, ptr),
        "tile: NULL buffer": lambda: hip.hrt_render_aov_tile(h, cb, pb, full, None),
        "tile: empty": lambda: hip.hrt_render_aov_tile(h, cb, pb, api.Rect(0, 0, 0, H), ptr),
        "tile: empty rows": lambda: hip.hrt_render_aov_tile(h, cb, pb, api.Rect(0, 0, W, 0), ptr),
        "tile: negative origin": lambda: hip.hrt_render_aov_tile(h, cb, pb, api.Rect(-1, 0, 4, 4), ptr),
        "tile: past the right edge": lambda: hip.hrt_render_aov_tile(h, cb, pb, api.Rect(W - 3, 0, 4, 4), ptr),
        "tile: past the bottom": lambda: hip.hrt_render_aov_tile(h, cb, pb, api.Rect(0, H - 3, 4, 4), ptr),
        "tile: samples 0": lambda: hip.hrt_render_aov_tile(h, cb, C.byref(_with(api, p, samples=0)), full, ptr),
        "stripes: NULL camera": lambda: hip.hrt_render_aov_stripes(h, None, pb, 4, 0, 1, ptr, 0, -1),
        "stripes: NULL params": lambda: hip.hrt_render_aov_stripes(h, cb, None, 4, 0, 1, ptr, 0, -1),
        "stripes: NULL buffer": lambda: hip.hrt_render_aov_stripes(h, cb, pb, 4, 0, 1, None, 0, -1),
        "stripes: sample_count 0": lambda: hip.hrt_render_aov_stripes(h, cb, pb, 4, 0, 1, ptr, 0, 0),
        "stripes: range past samples": lambda: hip.hrt_render_aov_stripes(h, cb, pb, 4, 0, 1, ptr, 2, spp - 1),
        "stripes: first == samples": lambda: hip.hrt_render_aov_stripes(h, cb, pb, 4, 0, 1, ptr, spp, -1),
        "stripes: negative first": lambda: hip.hrt_render_aov_stripes(h, cb, pb, 4, 0, 1, ptr, -1, 2),
        "stripes: rank == n_ranks": lambda: hip.hrt_render_aov_stripes(h, cb, pb, 4, 2, 2, ptr, 0, -1),
        "stripes: rows_per_block 0": lambda: hip.hrt_render_aov_stripes(h, cb, pb, 0, 0, 1, ptr, 0, -1),
        "device: NULL camera": lambda: hip.hrt_render_aov_stripes_device(h, None, pb, 4, 0, 1, dptr, 0, -1, None),
        "device: NULL params": lambda: hip.hrt_render_aov_stripes_device(h, cb, None, 4, 0, 1, dptr, 0, -1, None),
        "device: NULL buffer": lambda: hip.hrt_render_aov_stripes_device(h, cb, pb, 4, 0, 1, None, 0, -1, None),
        "device: sample_count 0": lambda: hip.hrt_render_aov_stripes_device(h, cb, pb, 4, 0, 1, dptr, 0, 0, None),
        "device: range past samples": lambda: hip.hrt_render_aov_stripes_device(h, cb, pb, 4, 0, 1, dptr, spp - 1, 2, None),
        "device: rank == n_ranks": lambda: hip.hrt_render_aov_stripes_device(h, cb, pb, 4, 1, 1, dptr, 0, -1, None),
        # (refused before anything is launched: the kernel's 16-byte loads and stores never see the pointer)
        "device: buffer not 16-byte aligned": lambda: hip.hrt_render_aov_stripes_device(h, cb, pb, 4, 0, 1, C.c_void_p(t.data_ptr() + 4), 0, -1, None),
        "device: buffer 8-byte aligned": lambda: hip.hrt_render_aov_stripes_device(h, cb, pb, 4, 0, 1, C.c_void_p(t.data_ptr() + 8), 1, 2, None),
    }
    for what, call in calls.items():
        assert call() == api.HRT_ERR_INVALID, what
        assert hip.hrt_last_error(), what
        assert (out == 7.0).all(), what
    torch.cuda.synchronize()
    assert bool((t == 7.0).all())
    with pytest.raises(api.HrtError) as e:
        dev.render_aov_tile(cam, p, (0, 0, W + 1, H))
    assert e.value.status == api.HRT_ERR_INVALID
    with pytest.raises(ValueError):                              # a continued accumulation needs the buffer it continues
        dev.render_aov_stripes(cam, p, 4, 0, 1, None, 2, 1)
    dev.render_aov_stripes(cam, p, 4, 0, 1, out, 0, -1)          # and a good call still works, on both buffers
    dev.render_aov_stripes_device(cam, p, 4, 0, 1, t.data_ptr())
    torch.cuda.synchronize()
    assert not (out == 7.0).all() and np.array_equal(_bits(t.cpu().numpy()), _bits(out))


def test_cli_aov(cornell, tmp_path, scenes_dir):
    import json
    api, hs, dev = cornell
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    W, H = 48, 32
    common = ["s.yaml", "--size", f"{W}x{H}", "--spp", "4", "--seed", "2", "--no-progress"]
    names = ("albedo", "normal", "depth", "alpha")

    def run(*extra):
        return subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=600)

    def files(prefix):
        return {n: (tmp_path / f"{prefix}.{n}.pfm").read_bytes() for n in names}
    r = run("--aov", "p", "--aov-spp", "2", "--dump-linear", "with.pfm", "--out", "a.png", "--stats")
    assert r.returncode == 1, r.stdout + r.stderr            # Film::outputFilm's 1 = success (Q-12)
    js = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert js["aov_spp"] == 2 and js["aov_s"] > 0 and js["samples"] == W * H * 4
    want = dev.render_aov_tile(hs.camera(W, H), api.default_params(W, H, 2, seed=2))
    got = {n: api.read_pfm(str(tmp_path / f"p.{n}.pfm")) for n in names}
    assert all(g.shape == (H, W, 3) for g in got.values())
    assert np.array_equal(_bits(got["albedo"]), _bits(want["albedo"])) and np.array_equal(_bits(got["normal"]), _bits(want["normal"]))
    for n in ("depth", "alpha"):                             # the scalars in all three channels
        assert np.array_equal(_bits(got[n]), _bits(np.repeat(want[n][..., None], 3, axis=2))), n
    assert 0 < want["alpha"].mean() and (want["depth"] > 0).any()
    ref = files("p")
    # the default count is min(spp, 16) ...
    r = run("--aov", "d", "--out", "d.png")
    assert r.returncode == 1, r.stderr
    want4 = dev.render_aov_tile(hs.camera(W, H), api.default_params(W, H, 4, seed=2))
    assert np.array_equal(_bits(api.read_pfm(str(tmp_path / "d.normal.pfm"))), _bits(want4["normal"]))
    # ... the same files whatever the estimator and the schedule of the film's render are ...
    r = run("--aov", "q", "--aov-spp", "2", "--nee", "--roulette", "--adaptive", "0.05", "--min-samples", "2", "--out", "q.png")
    assert r.returncode == 1, r.stderr
    assert files("q") == ref
    r = run("--aov", "c1", "--aov-spp", "2", "--progressive", "2", "--checkpoint", "ck", "--max-passes", "1", "--out", "c.png")
    assert r.returncode == 1, r.stderr
    assert files("c1") == ref
    r = run("--aov", "c2", "--aov-spp", "2", "--progressive", "2", "--checkpoint", "ck", "--resume", "--out", "c.png", "--dump-linear", "resumed.pfm")
    assert r.returncode == 1, r.stderr
    assert files("c2") == ref
    # ... but not whatever the lens, the sampler and the seed are
    for extra in (("--lens",), ("--stratified",), ("--seed", "3")):
        r = run("--aov", "x", "--aov-spp", "2", "--out", "x.png", *extra)
        assert r.returncode == 1, r.stderr
        assert files("x")["depth"] != ref["depth"], extra
    # usage errors
    for extra in (("--aov-spp", "0"), ("--aov-spp", "5"), ("--aov-spp", "-1"), ("--aov-spp", "x")):
        r = run("--aov", "u", "--out", "u.png", *extra)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "u.albedo.pfm").exists()
    r = run("--aov-spp", "2", "--out", "u.png")               # the count of a pass that was not asked for
    assert r.returncode == 2 and "--aov" in r.stderr, (r.returncode, r.stderr)
    # the film does not know the pass ran
    r = run("--dump-linear", "without.pfm", "--out", "b.png")
    assert r.returncode == 1, r.stderr
    assert (tmp_path / "without.pfm").read_bytes() == (tmp_path / "with.pfm").read_bytes() == (tmp_path / "resumed.pfm").read_bytes()
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes()
    assert not any((tmp_path / f"without.{n}.pfm").exists() for n in names)
