"""Environment-map importance sampling (HRT_FLAG_NEE_ENV) on the GPU: the device-built sampling table against numpy float64,
a floor under one bright block of the map against its closed-form irradiance, block means against the default estimator on the hall-map
scenes, the --nee film and counters on scenes without an environment map, every batching form bit for bit, the error at equal spp, the
refusals and the CLI."""
import os
import subprocess

import numpy as np
import pytest

from tests import env_tables as et

pytestmark = pytest.mark.gpu


def _report(line):
    """measurements (DESIGN.md 4.6 quotes them): printed, and appended to the file $HRT_NEE_REPORT names, if any"""
    print(line)
    path = os.environ.get("HRT_NEE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _scene(d, name, yaml):
    from hobbyraytracer_amd import api
    p = os.path.join(str(d), name + ".yaml")
    with open(p, "w") as f:
        f.write(yaml)
    return api.HostScene(p, str(d))


def _ulps(a, b):
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def _check_table(got, tex):
    ref = et.table(tex)
    assert got is not None and ref is not None
    for g, r in zip(got, ref):
        assert g.shape == r.shape
        assert (g[..., 0] == 0).all() and (g[..., -1] == 1).all()
        assert (np.diff(g, axis=-1) >= 0).all()
        assert _ulps(g, r).max() <= 1, np.argwhere(_ulps(g, r) > 1)[:5]


def test_table_build_matches_float64(built, tmp_path):
    from hobbyraytracer_amd import api
    api.write_hall_hdr(str(tmp_path / "hall.hdr"), 4096, 2048)
    hall = api.read_hdr(str(tmp_path / "hall.hdr"))
    _check_table(api.env_table_build(hall), hall)
    rng = np.random.default_rng(1)
    for W, H in ((1, 1), (1, 9), (13, 1), (2, 2), (37, 19), (300, 7), (1000, 300)):
        tex = et.messy_map(rng, W, H) if W > 2 and H > 2 else rng.gamma(0.6, 1.0, size=(H, W, 3)).astype(np.float32)
        _check_table(api.env_table_build(tex), tex)
    tex4 = np.concatenate([et.messy_map(rng, 50, 20), rng.random((20, 50, 1), np.float32)], axis=2)   # 4 channels: the 4th is ignored
    _check_table(api.env_table_build(tex4), tex4)
    for bad in (np.zeros((8, 16, 3), np.float32), np.full((8, 16, 3), np.nan, np.float32), np.full((8, 16, 3), -1.0, np.float32)):
        assert api.env_table_build(bad) is None


# ---------------------------------------------------------------- closed form: a diffuse floor under one bright block of the map
MAP_W, MAP_H, BLOCK_I, BLOCK_J, L_BLOCK, ALBEDO = 64, 32, (10, 20), (6, 12), 2.0, 0.5
FLOOR_YAML = f"""film:
    width: 32
    height: 32
    samples: 1
    output: out.png
camera:
    position: [0.1, 0.6, 0.05]
    look_at: [0.1, 0.0, 0.0501]
    up: [0, 0, -1]
    fov: 60
    aperture: 0
    focal_distance: 1
    background: sky
textures:
  - name: sky
    type: environment
    path: block.hdr
materials:
  - name: floor
    type: lambertian
    albedo: [{ALBEDO}, {ALBEDO}, {ALBEDO}]
objects:
  - type: xz_rect
    x: [-50, 50]
    z: [-50, 50]
    k: 0
    material: floor
"""


def _block_map():
    tex = np.zeros((MAP_H, MAP_W, 3), np.float32)
    tex[BLOCK_J[0]:BLOCK_J[1] + 1, BLOCK_I[0]:BLOCK_I[1] + 1] = L_BLOCK
    return tex


def _block_irradiance():
    """a / pi x L x dphi x (sin^2 theta_hi - sin^2 theta_lo) / 2 over the block's exact texel bounds"""
    (i0, i1), (j0, j1) = BLOCK_I, BLOCK_J
    dphi = 2 * np.pi * (i1 - i0 + 1) / (MAP_W - 1)
    th_lo, th_hi = np.pi * (j0 - 0.5) / (MAP_H - 1), np.pi * (j1 + 0.5) / (MAP_H - 1)
    return ALBEDO / np.pi * L_BLOCK * dphi * (np.sin(th_hi) ** 2 - np.sin(th_lo) ** 2) / 2


@pytest.fixture(scope="module")
def floor(built, tmp_path_factory):
    from hobbyraytracer_amd import api
    d = tmp_path_factory.mktemp("env_floor")
    api.write_hdr(str(d / "block.hdr"), _block_map())
    assert np.array_equal(api.read_hdr(str(d / "block.hdr")), _block_map())      # exact in RGBE
    hs = _scene(d, "floor", FLOOR_YAML)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


def test_floor_under_a_bright_block_matches_the_closed_form(floor):
    api, hs, dev = floor
    W = H = 32
    cam = hs.camera(W, H)
    pred = _block_irradiance()
    spread = {}
    for nee_env in (False, True):
        img, st = dev.render_tile(cam, api.default_params(W, H, 512, max_depth=2, seed=21, nee_env=nee_env))
        r = img[..., 0].astype(np.float64).reshape(-1) / pred   # grey floor, grey block: one channel (the three are the same draws)
        z = (r.mean() - 1.0) / (r.std(ddof=1) / np.sqrt(r.size))
        _report(f"env floor closed form nee_env={nee_env}: mean ratio {r.mean():.6f}, per-pixel std {r.std():.5f}, z {z:.2f}, "
                f"shadow_rays {st.shadow_rays}")
        assert abs(z) < 4.0, (nee_env, r.mean(), z)
        assert (st.shadow_rays > 0) == nee_env
        spread[nee_env] = r.std()
    _report(f"env floor: per-pixel spread ratio nee_env / default = {spread[True] / spread[False]:.4f}")
    assert spread[True] < 0.25 * spread[False], spread      # measured: 0.098


# ---------------------------------------------------------------- unbiasedness on the hall-map scenes
ENV_SCENE_YAML = """film:
    width: 64
    height: 64
    samples: 1
    output: out.png
camera:
    position: [0, 2.0, 6.5]
    look_at: [0, 0.8, 0]
    up: [0, 1, 0]
    fov: 50
    aperture: 0
    focal_distance: 1
    background: hall
textures:
  - name: hall
    type: environment
    path: old_hall_4k.hdr
materials:
  - name: grey
    type: lambertian
    albedo: [0.6, 0.6, 0.6]
  - name: red
    type: lambertian
    albedo: [0.7, 0.2, 0.15]
  - name: white
    type: lambertian
    albedo: [0.75, 0.75, 0.75]
  - name: lamp
    type: diffuse_light
    albedo: [1, 0.9, 0.8]
    strength: 4
objects:
  - type: xz_rect
    x: [-6, 6]
    z: [-6, 6]
    k: 0
    material: grey
  - type: sphere
    center: [-1.4, 0.7, 0.4]
    radius: 0.7
    material: red
  - type: xy_rect
    x: [0.8, 2.0]
    y: [1.8, 2.4]
    k: -1.5
    material: lamp
  - type: mesh
    path: teapot.obj
    material: white
    transform:
        rotate: [10, 40, 0]
        translate: [0.9, 0.6, 0]
        scale: [0.7, 0.7, 0.7]
"""


def _env_scene(assets, tmp_path):
    d = tmp_path / "env_scene"
    d.mkdir(exist_ok=True)
    for f in ("teapot.obj", "old_hall_4k.hdr"):
        if not (d / f).exists():
            os.symlink(os.path.join(assets, f), d / f)
    return _scene(d, "env_scene", ENV_SCENE_YAML)


def _block_stats(films):
    y = films @ np.array([0.2126, 0.7152, 0.0722])
    S, H, W = y.shape
    b = y.reshape(S, H // 16, 16, W // 16, 16).mean(axis=(2, 4))
    return b.mean(0), b.std(0, ddof=1) / np.sqrt(S)


def test_env_nee_is_unbiased_and_keeps_the_paths(built, assets, scenes_dir, tmp_path):
    from hobbyraytracer_amd import api
    W = H = 64
    seeds, spp = 16, 16
    scenes = {n: api.HostScene(os.path.join(scenes_dir, n + ".yaml"), assets) for n in ("teapot_scene", "shiny_teapot")}
    scenes["env_scene"] = _env_scene(assets, tmp_path)
    for name, hs in scenes.items():
        dev = api.DeviceScene(hs.flat_ptr, 0)
        try:
            cam = hs.camera(W, H)
            films = {False: [], True: []}
            for s in range(seeds):
                st_of = {}
                for env in (False, True):
                    img, st = dev.render_tile(cam, api.default_params(W, H, spp, seed=2000 + s, nee_env=env))
                    films[env].append(img)
                    st_of[env] = st
                assert st_of[True].rays == st_of[False].rays, name
                if name == "shiny_teapot":            # a metal teapot: no vertex is eligible, every escape keeps weight 1
                    assert np.array_equal(films[True][-1].view(np.uint32), films[False][-1].view(np.uint32))
                if s == 0:
                    _, st_nee = dev.render_tile(cam, api.default_params(W, H, spp, seed=2000, nee=True))
                    _report(f"{name}: rays {st_of[True].rays}, shadow_rays --nee {st_nee.shadow_rays}, --nee-env {st_of[True].shadow_rays}")
                    if name == "shiny_teapot":        # a metal teapot: no vertex is eligible
                        assert st_of[True].shadow_rays == st_nee.shadow_rays == 0
                    else:
                        assert st_of[True].shadow_rays > st_nee.shadow_rays, name
            if name == "shiny_teapot":
                continue                              # bit-equal films: nothing for a z-test to see
            (ma, sa), (mb, sb) = _block_stats(np.array(films[False], np.float64)), _block_stats(np.array(films[True], np.float64))
            z = (mb - ma) / np.sqrt(sa * sa + sb * sb + 1e-30)
            _report(f"{name}: max |z| of 16x16 block means --nee-env vs default = {np.abs(z).max():.2f}; "
                    f"mean block std error default {sa.mean():.4g}, --nee-env {sb.mean():.4g}")
            assert np.abs(z).max() < 5.0, (name, z)
        finally:
            dev.close()


@pytest.mark.parametrize("name", ["cornell_box", "material_zoo"])
def test_backgrounds_without_a_map_render_the_nee_film(built, assets, scenes_dir, name):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, name + ".yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        cam = hs.camera(40, 32)
        a, sa = dev.render_tile(cam, api.default_params(40, 32, 4, seed=9, nee=True, stats=True))
        b, sb = dev.render_tile(cam, api.default_params(40, 32, 4, seed=9, nee_env=True, stats=True))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for f in ("rays", "samples", "box_tests", "tri_tests", "mesh_hits", "env_lookups", "shadow_rays"):
            assert getattr(sa, f) == getattr(sb, f), f
    finally:
        dev.close()


@pytest.fixture(scope="module")
def teapot(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "teapot_scene.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


def test_env_nee_forms_agree_bit_for_bit(teapot):
    api, hs, dev = teapot
    W, H, spp = 48, 40, 6
    cam = hs.camera(W, H)
    p = api.default_params(W, H, spp, seed=3, nee_env=True)
    tile, st = dev.render_tile(cam, p)
    _, st_nee = dev.render_tile(cam, api.default_params(W, H, spp, seed=3, nee=True))
    assert st.shadow_rays > st_nee.shadow_rays
    for G in (1, 2, 4):
        film = np.zeros_like(tile)
        for rank in range(G):
            part, _ = dev.render_stripes(cam, p, 4, rank, G)
            rows = [api.stripe_row_index(H, 4, rank, G, i) for i in range(part.shape[0])]
            film[rows] = part
        assert np.array_equal(film.view(np.uint32), tile.view(np.uint32)), G
    one, _ = dev.render_stripes(cam, p, 8, 0, 1)
    acc = np.zeros_like(one)
    for first, n in ((0, 2), (2, 3), (5, 1)):
        dev.render_stripes_accumulate(cam, p, 8, 0, 1, acc, first, n)
    assert np.array_equal(acc.view(np.uint32), one.view(np.uint32))
    mean, count, _ = dev.render_adaptive(cam, p, api.Adaptive(2, 3, 0.0, 0.0))
    assert (count == spp).all()
    assert np.array_equal(mean.reshape(one.shape).view(np.uint32), one.view(np.uint32))
    films = []
    for devices in ((0,), (0, 0)):
        m = api.MultiScene(hs.flat_ptr, devices=devices, loopback=True)
        try:
            sums, _, _ = m.render(cam, p, rows_per_block=8, want_u8=False)
        finally:
            m.close()
        films.append(sums)
    assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32))
    assert np.array_equal(films[0].view(np.uint32), tile.view(np.uint32))


def test_env_nee_lowers_the_error(built, assets, tmp_path):
    from hobbyraytracer_amd import api
    hs = _env_scene(assets, tmp_path)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        W = H = 64
        spp = 16
        cam = hs.camera(W, H)
        ref = np.zeros((H, W, 3))
        for env in (False, True):    # the reference: --nee and --nee-env at 8 x spp, other seeds
            img, _ = dev.render_tile(cam, api.default_params(W, H, 8 * spp, seed=77, nee=True, nee_env=env))
            ref += 0.5 * img
        rms = {}
        for env in (False, True):
            err = []
            for s in range(4):
                img, _ = dev.render_tile(cam, api.default_params(W, H, spp, seed=500 + s, nee=True, nee_env=env))
                err.append(np.mean((img - ref) ** 2))
            rms[env] = float(np.sqrt(np.mean(err)))
        _report(f"env_scene 64x64 {spp} spp RMS vs {8 * spp}-spp reference: --nee {rms[False]:.5f}, --nee-env {rms[True]:.5f}, "
                f"ratio {rms[True] / rms[False]:.3f}")
        assert rms[True] <= 0.4 * rms[False], rms            # measured: 0.215
    finally:
        dev.close()


def test_refusals(teapot):
    api, hs, dev = teapot
    with pytest.raises(api.HrtError) as e:
        dev.render_tile(hs.camera(16, 16), api.default_params(16, 16, 1, megakernel=True, nee_env=True))
    assert e.value.status == api.HRT_ERR_UNSUPPORTED
    p = api.default_params(16, 16, 1)
    p.flags |= api.FLAG_NEE_ENV                   # without FLAG_NEE
    with pytest.raises(api.HrtError) as e:
        dev.render_tile(hs.camera(16, 16), p)
    assert e.value.status == api.HRT_ERR_INVALID


def test_cli_nee_env_and_cross_mode_resume(built, assets, scenes_dir, tmp_path):
    from hobbyraytracer_amd import api
    with open(os.path.join(scenes_dir, "teapot_scene.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    for a in ("teapot.obj", "old_hall_4k.hdr"):
        os.symlink(os.path.join(assets, a), tmp_path / a)
    common = ["s.yaml", "--size", "48x32", "--spp", "4", "--seed", "2", "--no-progress", "--assets", str(tmp_path)]

    def run(*extra):
        return subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    p = run("--nee-env", "--out", "env.png", "--stats")
    assert p.returncode == 1, p.stderr             # Film::outputFilm's 1 = success (Q-12)
    assert (tmp_path / "env.png").exists() and '"shadow_rays"' in p.stdout
    p = run("--nee-env", "--out", "a.png", "--progressive", "2", "--checkpoint", "env.ck", "--max-passes", "1")
    assert p.returncode == 1, p.stderr
    p = run("--nee", "--out", "a.png", "--progressive", "2", "--checkpoint", "env.ck", "--resume")
    assert p.returncode != 1 and "different render" in p.stderr
    p = run("--nee", "--out", "b.png", "--progressive", "2", "--checkpoint", "nee.ck", "--max-passes", "1")
    assert p.returncode == 1, p.stderr
    p = run("--nee-env", "--out", "b.png", "--progressive", "2", "--checkpoint", "nee.ck", "--resume")
    assert p.returncode != 1 and "different render" in p.stderr
    p = run("--nee-env", "--out", "c.png", "--progressive", "2", "--checkpoint", "env.ck", "--resume")
    assert p.returncode == 1, p.stderr
