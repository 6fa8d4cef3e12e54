"""Light sampling at rough metal and medium vertices (HRT_FLAG_NEE_LOBES) on the GPU: with the flag the film agrees
with the default estimator's (block means, z-scores) and the paths are the default render's (the `rays` counter); every batching,
striping, adaptive and multi-GPU form gives the same bits; where only Lambertian vertices are eligible the film is --nee's bit for
bit; it lowers the error where the light is found from fog or from a brushed-metal floor; the megakernel refuses it."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _report(line):
    """measurements (DESIGN.md 4.8 quotes them): printed, and appended to the file $HRT_NEE_REPORT names, if any"""
    print(line)
    path = os.environ.get("HRT_NEE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _scene(tmp_path, name, yaml, assets=None):
    from hobbyraytracer_amd import api
    p = os.path.join(str(tmp_path), name + ".yaml")
    with open(p, "w") as f:
        f.write(yaml)
    return api.HostScene(p, assets or str(tmp_path))


_HEAD = """film:
    width: 64
    height: 64
    samples: 1
    output: out.png
"""

# A Lambertian room filled with fog (the medium's boundary lies just inside the walls; the camera stands in it) and a small lamp
# under the ceiling, above and behind the camera's view: a path that scatters in the fog finds the lamp only by luck.
FOG_ROOM_YAML = _HEAD + """camera:
    position: [0, 1.4, 1.9]
    look_at: [0, 1.3, -1]
    up: [0, 1, 0]
    fov: 70
    aperture: 0
    focal_distance: 1
    background: [0, 0, 0]
materials:
  - name: white
    type: lambertian
    albedo: [0.7, 0.7, 0.7]
  - name: green
    type: lambertian
    albedo: [0.2, 0.6, 0.25]
  - name: lamp
    type: diffuse_light
    albedo: [1, 0.9, 0.8]
    strength: 160
objects:
  - type: constant_medium
    density: 0.35
    colour: [0.9, 0.9, 0.95]
    boundary:
        type: box
        min: [-1.99, 0.01, -1.99]
        max: [1.99, 2.95, 1.99]
  - type: xz_rect
    x: [-2, 2]
    z: [-2, 2]
    k: 0
    material: white
  - type: xz_rect
    x: [-2, 2]
    z: [-2, 2]
    k: 3
    material: white
  - type: xy_rect
    x: [-2, 2]
    y: [0, 3]
    k: -2
    material: white
  - type: xy_rect
    x: [-2, 2]
    y: [0, 3]
    k: 2
    material: white
  - type: yz_rect
    y: [0, 3]
    z: [-2, 2]
    k: -2
    material: green
  - type: yz_rect
    y: [0, 3]
    z: [-2, 2]
    k: 2
    material: white
  - type: xz_rect
    x: [-0.1, 0.1]
    z: [0.9, 1.1]
    k: 2.94
    material: lamp
"""

# A brushed-metal floor (roughness 0.5) under a small lamp whose glossy reflection lies in view, with a teapot under a scaling transform (a wrapped mesh: quirk Q-1 makes
# its t depend on the ray's length) standing between the lamp and part of the floor.
BRUSHED_FLOOR_YAML = _HEAD + """camera:
    position: [0, 2.2, 6.0]
    look_at: [0, 0.6, 0]
    up: [0, 1, 0]
    fov: 40
    aperture: 0
    focal_distance: 1
    background: [0, 0, 0]
materials:
  - name: brushed
    type: metal
    albedo: [0.8, 0.75, 0.7]
    roughness: 0.5
  - name: white
    type: lambertian
    albedo: [0.7, 0.7, 0.7]
  - name: light
    type: diffuse_light
    albedo: [1, 0.9, 0.8]
    strength: 17
objects:
  - type: xz_rect
    x: [-4, 4]
    z: [-4, 4]
    k: 0
    material: brushed
  - type: xz_rect
    x: [-0.4, 0.4]
    z: [-3.4, -2.6]
    k: 2.0
    material: light
  - type: mesh
    path: teapot.obj
    material: white
    transform:
        rotate: [20, 35, 10]
        translate: [0, 1.1, -0.6]
        scale: [0.9, 1.3, 0.8]
"""

# Lambertian only (tests/test_gpu_nee.py's mesh-shadow scene without the mesh): the flag must change nothing against --nee
LAMBERT_YAML = _HEAD + """camera:
    position: [0, 3.0, 6.0]
    look_at: [0, 0.5, 0]
    up: [0, 1, 0]
    fov: 40
    aperture: 0
    focal_distance: 1
    background: [0, 0, 0]
materials:
  - name: white
    type: lambertian
    albedo: [0.7, 0.7, 0.7]
  - name: light
    type: diffuse_light
    albedo: [1, 0.9, 0.8]
    strength: 6
objects:
  - type: xz_rect
    x: [-4, 4]
    z: [-4, 4]
    k: 0
    material: white
  - type: xy_rect
    x: [-4, 4]
    y: [0, 4]
    k: -2
    material: white
  - type: xz_rect
    x: [-0.6, 0.6]
    z: [-0.6, 0.6]
    k: 3.5
    material: light
  - type: sphere
    center: [0.8, 0.6, 0.5]
    radius: 0.6
    material: white
"""


def _with_teapot(tmp_path, assets, name, yaml):
    d = tmp_path / name
    d.mkdir()
    with open(os.path.join(assets, "teapot.obj")) as f:
        (d / "teapot.obj").write_text(f.read())
    return _scene(d, name, yaml)


@pytest.fixture(scope="module")
def fog_room(built, tmp_path_factory):
    from hobbyraytracer_amd import api
    hs = _scene(tmp_path_factory.mktemp("fog_room"), "fog_room", FOG_ROOM_YAML)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


@pytest.fixture(scope="module")
def brushed_floor(built, assets, tmp_path_factory):
    from hobbyraytracer_amd import api
    hs = _with_teapot(tmp_path_factory.mktemp("brushed"), assets, "brushed_floor", BRUSHED_FLOOR_YAML)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


def _block_stats(films):
    """films [S, H, W, 3] of S seeds -> (mean of 16x16 block luminance means, its standard error) per block"""
    y = films @ np.array([0.2126, 0.7152, 0.0722])
    S, H, W = y.shape
    b = y.reshape(S, H // 16, 16, W // 16, 16).mean(axis=(2, 4))
    return b.mean(0), b.std(0, ddof=1) / np.sqrt(S)


def _unbiased(name, dev, cam, flags):
    """the 16-seed, 16 spp, 64x64, 16x16-block z-test of tests/test_gpu_nee.py: `flags` on against the default estimator"""
    from hobbyraytracer_amd import api
    W = H = 64
    seeds, spp = 16, 16
    films = {False: [], True: []}
    for s in range(seeds):
        st_of = {}
        for on in (False, True):
            p = api.default_params(W, H, spp, seed=1000 + s, **(flags if on else {}))
            img, st = dev.render_tile(cam, p)
            films[on].append(img.astype(np.float64))
            st_of[on] = st
        assert st_of[True].rays == st_of[False].rays, name          # the path vertices are the default render's
        assert st_of[False].shadow_rays == 0 and st_of[True].shadow_rays > 0, name
        if s == 0:
            _report(f"{name} {sorted(flags)}: rays {st_of[True].rays}, shadow_rays {st_of[True].shadow_rays}")
    (ma, sa), (mb, sb) = _block_stats(np.array(films[False])), _block_stats(np.array(films[True]))
    z = (mb - ma) / np.sqrt(sa * sa + sb * sb + 1e-30)
    _report(f"{name} {sorted(flags)}: max |z| of 16x16 block means vs default = {np.abs(z).max():.2f} "
            f"(z = {z.flat[np.abs(z).argmax()]:.4f} in block {tuple(int(i) for i in np.unravel_index(np.abs(z).argmax(), z.shape))}); "
            f"mean block std error default {sa.mean():.4g}, with the flags {sb.mean():.4g}")
    assert np.abs(z).max() < 5.0, (name, z)


@pytest.mark.parametrize("name,flags", [("material_zoo", dict(nee_lobes=True)), ("bust_scene", dict(nee_lobes=True)),
                                        ("shiny_teapot", dict(nee_env=True, nee_lobes=True)),
                                        ("material_zoo", dict(nee_emitters=True, nee_lobes=True))])
def test_lobes_are_unbiased_on_the_golden_scenes(built, assets, scenes_dir, name, flags):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, name + ".yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        _unbiased(name, dev, hs.camera(64, 64), flags)
    finally:
        dev.close()


def test_lobes_are_unbiased_in_the_fog_room(fog_room):
    api, hs, dev = fog_room
    _unbiased("fog_room", dev, hs.camera(64, 64), dict(nee_lobes=True))
    _unbiased("fog_room", dev, hs.camera(64, 64), dict(nee_emitters=True, nee_lobes=True))


def test_lobes_are_unbiased_on_the_brushed_floor(brushed_floor):
    api, hs, dev = brushed_floor
    _unbiased("brushed_floor", dev, hs.camera(64, 64), dict(nee_lobes=True))


def test_lobes_forms_agree_bit_for_bit(fog_room):
    api, hs, dev = fog_room
    W, H, spp = 48, 40, 6
    cam = hs.camera(W, H)
    p = api.default_params(W, H, spp, seed=3, nee_lobes=True)
    tile, st = dev.render_tile(cam, p)
    plain, st_n = dev.render_tile(cam, api.default_params(W, H, spp, seed=3, nee=True))
    assert st.shadow_rays > st_n.shadow_rays > 0 and not np.array_equal(tile, plain)   # the fog's vertices take samples too
    for G in (1, 2, 4):                                       # stripes of 1, 2 and 4 ranks
        film = np.zeros_like(tile)
        for rank in range(G):
            part, _ = dev.render_stripes(cam, p, 4, rank, G)
            rows = [api.stripe_row_index(H, 4, rank, G, i) for i in range(part.shape[0])]
            film[rows] = part
        assert np.array_equal(film.view(np.uint32), tile.view(np.uint32)), G
    one, _ = dev.render_stripes(cam, p, 8, 0, 1)              # progressive batches 2 + 3 + 1 against one shot
    acc = np.zeros_like(one)
    for first, n in ((0, 2), (2, 3), (5, 1)):
        dev.render_stripes_accumulate(cam, p, 8, 0, 1, acc, first, n)
    assert np.array_equal(acc.view(np.uint32), one.view(np.uint32))
    mean, count, _ = dev.render_adaptive(cam, p, api.Adaptive(2, 3, 0.0, 0.0))   # adaptive with threshold 0 = uniform
    assert (count == spp).all()
    assert np.array_equal(mean.reshape(one.shape).view(np.uint32), one.view(np.uint32))
    films = []                                                # loopback multi-GPU session: G = 2 on one device equals G = 1
    for devices in ((0,), (0, 0)):
        m = api.MultiScene(hs.flat_ptr, devices=devices, loopback=True)
        try:
            sums, _, _ = m.render(cam, p, rows_per_block=8, want_u8=False)
        finally:
            m.close()
        films.append(sums)
    assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32))
    assert np.array_equal(films[0].view(np.uint32), tile.view(np.uint32))


def test_lambertian_only_scene_renders_the_nee_film(built, tmp_path):
    from hobbyraytracer_amd import api
    hs = _scene(tmp_path, "lambert", LAMBERT_YAML)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        cam = hs.camera(48, 40)
        for extra in (dict(), dict(nee_emitters=True)):
            a, sa = dev.render_tile(cam, api.default_params(48, 40, 6, seed=9, nee=True, **extra))
            b, sb = dev.render_tile(cam, api.default_params(48, 40, 6, seed=9, nee_lobes=True, **extra))
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), extra
            assert sa.rays == sb.rays and sa.shadow_rays == sb.shadow_rays > 0
    finally:
        dev.close()


def test_flag_without_anything_to_sample_renders_the_default_film(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "shiny_teapot.yaml"), assets)      # no table light: --nee --nee-lobes has no light to sample
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        cam = hs.camera(40, 32)
        a, sa = dev.render_tile(cam, api.default_params(40, 32, 4, seed=9))
        b, sb = dev.render_tile(cam, api.default_params(40, 32, 4, seed=9, nee_lobes=True))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert sa.rays == sb.rays and sb.shadow_rays == 0
    finally:
        dev.close()


def test_megakernel_and_lone_flag_are_refused(fog_room):
    api, hs, dev = fog_room
    with pytest.raises(api.HrtError) as e:
        dev.render_tile(hs.camera(16, 16), api.default_params(16, 16, 1, megakernel=True, nee_lobes=True))
    assert e.value.status == api.HRT_ERR_UNSUPPORTED
    p = api.default_params(16, 16, 1)
    p.flags |= api.FLAG_NEE_LOBES                          # without FLAG_NEE
    with pytest.raises(api.HrtError) as e:
        dev.render_tile(hs.camera(16, 16), p)
    assert e.value.status == api.HRT_ERR_INVALID
    assert api.default_params(16, 16, 1, nee_lobes=True).flags & api.FLAG_NEE


# Measured on the MI355X: RMS of 16-spp films against the 128-spp mean of both estimators, --nee --nee-lobes over --nee.
MEASURED_RATIO = {"fog_room": 0.408, "brushed_floor": 0.259}


def _rms_ratio(name, api, hs, dev):
    W = H = 64
    cam = hs.camera(W, H)
    ref = np.zeros((H, W, 3))
    for lobes in (False, True):     # the reference: both estimators at 8 x 16 spp, other seeds
        img, _ = dev.render_tile(cam, api.default_params(W, H, 128, seed=77, nee=True, nee_lobes=lobes))
        ref += 0.5 * img
    rms = {}
    for lobes in (False, True):
        err = []
        for s in range(4):
            img, _ = dev.render_tile(cam, api.default_params(W, H, 16, seed=500 + s, nee=True, nee_lobes=lobes))
            err.append(np.mean((img - ref) ** 2))
        rms[lobes] = float(np.sqrt(np.mean(err)))
    ratio = rms[True] / rms[False]
    _report(f"{name} 64x64 16 spp RMS vs 128-spp reference: --nee {rms[False]:.5f}, --nee --nee-lobes {rms[True]:.5f}, ratio {ratio:.3f}")
    return ratio


def test_lobes_lower_the_error_in_the_fog_room(fog_room):
    ratio = _rms_ratio("fog_room", *fog_room)
    assert MEASURED_RATIO["fog_room"] is not None and MEASURED_RATIO["fog_room"] <= 0.7
    assert ratio <= min(0.9, 1.3 * MEASURED_RATIO["fog_room"]), ratio


def test_lobes_lower_the_error_on_the_brushed_floor(brushed_floor):
    ratio = _rms_ratio("brushed_floor", *brushed_floor)
    assert MEASURED_RATIO["brushed_floor"] is not None and MEASURED_RATIO["brushed_floor"] <= 0.7
    assert ratio <= min(0.9, 1.3 * MEASURED_RATIO["brushed_floor"]), ratio


def test_cli_nee_lobes_and_cross_flag_resume(built, tmp_path):
    from hobbyraytracer_amd import api
    (tmp_path / "s.yaml").write_text(FOG_ROOM_YAML)
    common = ["s.yaml", "--size", "48x32", "--spp", "4", "--seed", "2", "--no-progress"]

    def run(*extra):
        return subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    p = run("--nee-lobes", "--out", "lobes.png", "--stats", "--dump-linear", "lobes.pfm")      # implies --nee
    assert p.returncode == 1, p.stderr             # Film::outputFilm's 1 = success (Q-12)
    assert (tmp_path / "lobes.png").exists() and '"shadow_rays"' in p.stdout
    p = run("--nee", "--out", "nee.png", "--dump-linear", "nee.pfm")
    assert p.returncode == 1, p.stderr
    assert (tmp_path / "lobes.pfm").read_bytes() != (tmp_path / "nee.pfm").read_bytes()
    # a checkpoint written with --nee-lobes cannot be continued by --nee alone, and the reverse
    p = run("--nee-lobes", "--out", "a.png", "--progressive", "2", "--checkpoint", "lobes.ck", "--max-passes", "1")
    assert p.returncode == 1, p.stderr
    p = run("--nee", "--out", "a.png", "--progressive", "2", "--checkpoint", "lobes.ck", "--resume")
    assert p.returncode != 1 and "different render" in p.stderr
    p = run("--nee", "--out", "b.png", "--progressive", "2", "--checkpoint", "nee.ck", "--max-passes", "1")
    assert p.returncode == 1, p.stderr
    p = run("--nee", "--nee-lobes", "--out", "b.png", "--progressive", "2", "--checkpoint", "nee.ck", "--resume")
    assert p.returncode != 1 and "different render" in p.stderr
    p = run("--nee-lobes", "--out", "c.png", "--progressive", "2", "--checkpoint", "lobes.ck", "--resume")
    assert p.returncode == 1, p.stderr
