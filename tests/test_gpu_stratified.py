"""The stratified sampler (HRT_FLAG_STRATIFIED) on the GPU: the device's draw is the host's word for word; the film is
unbiased against the default sampler's (block means, z-scores), with and without the NEE flags; every batching, striping, adaptive and
multi-GPU form gives the same bits; the megakernel refuses it; the CLI renders it and keeps its checkpoints apart; and on the floor
under a rect light, whose irradiance has a closed form, it lowers the error at equal sample count."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_stratified_cpu import STRAT, draws, lib  # noqa: F401  (the module-scoped fixture: one g++ run)

pytestmark = pytest.mark.gpu

# What tests/tools/stratified_time.py --error measured for the floor scene below: r = RMS_stratified / RMS_default against
# the closed form at 16 spp over the seeds 0..7, and the standard deviation of r over 8 disjoint groups of 8 seeds.
R_MEASURED, R_SPREAD = 0.2482, 0.0014


def _report(line):
    """measurements (DESIGN.md 4.9 quotes them): printed, and appended to the file $HRT_STRAT_REPORT names, if any"""
    print(line)
    path = os.environ.get("HRT_STRAT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _scene(tmp_path, name, yaml, assets=None):
    from hobbyraytracer_amd import api
    p = os.path.join(str(tmp_path), name + ".yaml")
    with open(p, "w") as f:
        f.write(yaml)
    return api.HostScene(p, assets or str(tmp_path))


# The scenes of tests/test_gpu_nee.py, restated: the floor under a rect light (closed form), a mesh that casts a shadow, mixed lights.
H_LIGHT, HALF, ALBEDO, LE = 1.0, 0.5, 0.5, (0.9, 0.8, 0.7)
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
    background: [0, 0, 0]
materials:
  - name: floor
    type: lambertian
    albedo: [{ALBEDO}, {ALBEDO}, {ALBEDO}]
  - name: lamp
    type: diffuse_light
    albedo: [{LE[0]}, {LE[1]}, {LE[2]}]
    strength: 1
objects:
  - type: xz_rect
    x: [-50, 50]
    z: [-50, 50]
    k: 0
    material: floor
  - type: xz_rect
    x: [{-HALF}, {HALF}]
    z: [{-HALF}, {HALF}]
    k: {H_LIGHT}
    material: lamp
"""


def _form_factor(x, z):
    """point-to-parallel-rectangle form factor of the light seen from floor point (x, 0, z) (sum over the four corner rectangles)"""
    def corner(a, b):
        A, B = a / H_LIGHT, b / H_LIGHT
        sa, sb = np.sqrt(1 + A * A), np.sqrt(1 + B * B)
        return (A / sa * np.arctan(B / sa) + B / sb * np.arctan(A / sb)) / (2 * np.pi)
    f = 0.0
    for sx, ex in ((1, HALF - x), (-1, -HALF - x)):
        for sz, ez in ((1, HALF - z), (-1, -HALF - z)):
            f = f + sx * sz * np.sign(ex) * np.sign(ez) * corner(np.abs(ex), np.abs(ez))
    return f


MESH_SHADOW_YAML = """film:
    width: 64
    height: 64
    samples: 1
    output: out.png
camera:
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
  - type: xz_rect
    x: [-0.6, 0.6]
    z: [-0.6, 0.6]
    k: 3.5
    material: light
  - type: mesh
    path: teapot.obj
    material: white
    transform:
        rotate: [20, 35, 10]
        translate: [0, 1.2, 0]
        scale: [0.9, 1.3, 0.8]
"""

MIXED_LIGHTS_YAML = """film:
    width: 64
    height: 64
    samples: 1
    output: out.png
camera:
    position: [0, 2.2, 6.5]
    look_at: [0, 1.0, 0]
    up: [0, 1, 0]
    fov: 45
    aperture: 0
    focal_distance: 1
    background: [0, 0, 0]
materials:
  - name: grey
    type: lambertian
    albedo: [0.6, 0.6, 0.6]
  - name: red
    type: lambertian
    albedo: [0.7, 0.2, 0.15]
  - name: mirror
    type: metal
    albedo: [0.8, 0.8, 0.8]
    roughness: 0.2
  - name: panel
    type: diffuse_light
    albedo: [1, 0.95, 0.9]
    strength: 3
  - name: bulb
    type: diffuse_light
    albedo: [0.4, 0.6, 1.0]
    strength: 12
  - name: tri_lamp
    type: diffuse_light
    albedo: [1, 0.5, 0.2]
    strength: 4
objects:
  - type: xz_rect
    x: [-4, 4]
    z: [-4, 4]
    k: 0
    material: grey
  - type: xy_rect
    x: [-4, 4]
    y: [0, 4]
    k: -2
    material: grey
  - type: xz_rect
    x: [-0.5, 0.5]
    z: [-0.5, 0.5]
    k: 3
    material: panel
  - type: sphere
    center: [1.8, 1.2, -0.5]
    radius: 0.35
    material: bulb
  - type: sphere
    center: [-0.6, 0.6, 0.3]
    radius: 0.6
    material: red
  - type: sphere
    center: [0.8, 0.45, 0.9]
    radius: 0.45
    material: mirror
  - type: triangle
    v0: [-2.5, 0.2, -1.5]
    v1: [-1.5, 0.2, -1.0]
    v2: [-2.0, 1.6, -1.3]
    material: tri_lamp
  - type: triangle
    v0: [-2.5, 0.2, -1.5]
    v1: [-2.0, 1.6, -1.3]
    v2: [-1.5, 0.2, -1.0]
    material: tri_lamp
"""


def _block_stats(films):
    """films [S, H, W, 3] of S seeds -> (mean of 16x16 block luminance means, its standard error) per block"""
    y = films @ np.array([0.2126, 0.7152, 0.0722])
    S, H, W = y.shape
    b = y.reshape(S, H // 16, 16, W // 16, 16).mean(axis=(2, 4))
    return b.mean(0), b.std(0, ddof=1) / np.sqrt(S)


def test_the_device_draw_is_the_host_draw(built, lib):  # noqa: F811
    from hobbyraytracer_amd import api
    rng = np.random.default_rng(2024)
    n = 120_000
    keys = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    keys[: n // 2, 1] &= np.uint32(0xFFFF)                      # sample indexes a render takes ...
    keys[: n // 2, 2] &= np.uint32(63)                          # ... bounces ...
    purpose = rng.choice([0, 1, 5, 6, 7], n // 2).astype(np.uint32)
    keys[: n // 2, 3] = purpose | (rng.integers(0, 2, n // 2).astype(np.uint32) << np.uint32(8))   # ... and sites; the other half: any 32 bits
    seed = 0x0123456789ABCDEF
    got = api.sampler_probe(seed, keys)
    want = np.zeros_like(keys)
    lib.sampler_draw(seed & 0xFFFFFFFF, seed >> 32, n, keys, want, STRAT)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def _five_scenes(assets, scenes_dir, tmp_path):
    from hobbyraytracer_amd import api
    out = {}
    for name in ("cornell_box", "material_zoo", "teapot_scene"):
        out[name] = api.HostScene(os.path.join(scenes_dir, name + ".yaml"), assets)
    with open(os.path.join(assets, "teapot.obj")) as f:
        obj = f.read()
    d = tmp_path / "mesh_shadow"
    d.mkdir()
    (d / "teapot.obj").write_text(obj)
    out["mesh_shadow"] = _scene(d, "mesh_shadow", MESH_SHADOW_YAML)
    d = tmp_path / "mixed_lights"
    d.mkdir()
    out["mixed_lights"] = _scene(d, "mixed_lights", MIXED_LIGHTS_YAML)
    return out


@pytest.mark.parametrize("flags", [dict(), dict(nee_lobes=True, nee_env=True, nee_emitters=True)], ids=["plain", "nee_all"])
def test_stratified_is_unbiased(built, assets, scenes_dir, tmp_path, flags):
    from hobbyraytracer_amd import api
    W = H = 64
    seeds, spp = 16, 16
    for name, hs in _five_scenes(assets, scenes_dir, tmp_path).items():
        dev = api.DeviceScene(hs.flat_ptr, 0)
        try:
            cam = hs.camera(W, H)
            films = {False: [], True: []}
            for s in range(seeds):
                for strat in (False, True):
                    img, st = dev.render_tile(cam, api.default_params(W, H, spp, seed=1000 + s, stratified=strat, **flags))   # reference quirks
                    films[strat].append(img.astype(np.float64))
            assert not np.array_equal(films[False][0], films[True][0]), name         # the flag draws other numbers
            (ma, sa), (mb, sb) = _block_stats(np.array(films[False])), _block_stats(np.array(films[True]))
            z = (mb - ma) / np.sqrt(sa * sa + sb * sb + 1e-30)
            _report(f"{name} {sorted(flags)}: max |z| of 16x16 block means stratified vs default = {np.abs(z).max():.2f}; "
                    f"mean block std error default {sa.mean():.4g}, stratified {sb.mean():.4g}")
            assert np.abs(z).max() < 5.0, (name, z)
        finally:
            dev.close()


@pytest.fixture(scope="module")
def cornell(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    hs = api.HostScene(os.path.join(scenes_dir, "cornell_box.yaml"), assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    yield api, hs, dev
    dev.close()


def test_stratified_forms_agree_bit_for_bit(cornell):
    api, hs, dev = cornell
    W, H, spp = 48, 40, 6
    cam = hs.camera(W, H)
    p = api.default_params(W, H, spp, seed=3, nee=True, stratified=True)
    tile, st = dev.render_tile(cam, p)
    assert st.shadow_rays > 0
    plain, _ = dev.render_tile(cam, api.default_params(W, H, spp, seed=3, nee=True))
    assert not np.array_equal(tile, plain)
    # stripes of 1, 2 and 4 ranks
    for G in (1, 2, 4):
        film = np.zeros_like(tile)
        for rank in range(G):
            part, _ = dev.render_stripes(cam, p, 4, rank, G)
            rows = [api.stripe_row_index(H, 4, rank, G, i) for i in range(part.shape[0])]
            film[rows] = part
        assert np.array_equal(film.view(np.uint32), tile.view(np.uint32)), G
    # progressive batches 2 + 3 + 1 against one shot
    one, _ = dev.render_stripes(cam, p, 8, 0, 1)
    acc = np.zeros_like(one)
    for first, n in ((0, 2), (2, 3), (5, 1)):
        dev.render_stripes_accumulate(cam, p, 8, 0, 1, acc, first, n)
    assert np.array_equal(acc.view(np.uint32), one.view(np.uint32))
    # adaptive with threshold 0 = uniform
    mean, count, _ = dev.render_adaptive(cam, p, api.Adaptive(2, 3, 0.0, 0.0))
    assert (count == spp).all()
    assert np.array_equal(mean.reshape(one.shape).view(np.uint32), one.view(np.uint32))
    # loopback multi-GPU session: G = 2 on one device equals G = 1
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


def test_the_default_film_does_not_know_the_flag_exists(cornell):
    """stats, thin lens and the counters variants: the flag off is the render it always was (films.npz pins it elsewhere); the flag on
    keeps the stats build and the plain build on the same film"""
    api, hs, dev = cornell
    cam = hs.camera(40, 32)
    a, sa = dev.render_tile(cam, api.default_params(40, 32, 4, seed=9, nee=True, stratified=True, thin_lens=True))
    b, sb = dev.render_tile(cam, api.default_params(40, 32, 4, seed=9, nee=True, stratified=True, thin_lens=True, stats=True))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and sa.rays == sb.rays and sa.shadow_rays == sb.shadow_rays


def test_megakernel_refuses_stratified(cornell):
    api, hs, dev = cornell
    with pytest.raises(api.HrtError) as e:
        dev.render_tile(hs.camera(16, 16), api.default_params(16, 16, 1, megakernel=True, stratified=True))
    assert e.value.status == api.HRT_ERR_UNSUPPORTED


def test_cli_stratified_and_cross_mode_resume(built, assets, scenes_dir, tmp_path):
    from hobbyraytracer_amd import api
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    common = ["s.yaml", "--size", "48x32", "--spp", "4", "--seed", "2", "--no-progress"]

    def run(*extra):
        return subprocess.run([api.CLI_PATH, *common, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    p = run("--stratified", "--out", "st.png", "--dump-linear", "st.pfm")
    assert p.returncode == 1, p.stderr             # Film::outputFilm's 1 = success (Q-12)
    p = run("--out", "plain.png", "--dump-linear", "plain.pfm")
    assert p.returncode == 1, p.stderr
    assert (tmp_path / "st.png").exists() and (tmp_path / "st.pfm").read_bytes() != (tmp_path / "plain.pfm").read_bytes()
    p = run("--stratified", "--nee", "--adaptive", "0.05", "--min-samples", "2", "--out", "ad.png")
    assert p.returncode == 1, p.stderr
    # a checkpoint written with --stratified cannot be continued without it, and the reverse
    p = run("--stratified", "--out", "a.png", "--progressive", "2", "--checkpoint", "st.ck", "--max-passes", "1")
    assert p.returncode == 1, p.stderr
    p = run("--out", "a.png", "--progressive", "2", "--checkpoint", "st.ck", "--resume")
    assert p.returncode != 1 and "different render" in p.stderr
    p = run("--out", "b.png", "--progressive", "2", "--checkpoint", "plain.ck", "--max-passes", "1")
    assert p.returncode == 1, p.stderr
    p = run("--stratified", "--out", "b.png", "--progressive", "2", "--checkpoint", "plain.ck", "--resume")
    assert p.returncode != 1 and "different render" in p.stderr
    p = run("--stratified", "--out", "c.png", "--progressive", "2", "--checkpoint", "st.ck", "--resume", "--dump-linear", "c.pfm")
    assert p.returncode == 1, p.stderr
    assert (tmp_path / "c.pfm").read_bytes() == (tmp_path / "st.pfm").read_bytes()      # resumed = one shot, bit for bit


# ------------------------------------------------------------------ the error against a closed form
def floor_prediction(cam, W, H, sub=4):
    """albedo Le F per pixel, F = the light's form factor averaged over sub x sub points of the pixel's footprint on the floor"""
    o = np.array(cam.origin, np.float64)
    llc, hor, ver = (np.array(v, np.float64) for v in (cam.lower_left, cam.horizontal, cam.vertical))
    x, row = np.meshgrid(np.arange(W), np.arange(H))
    f = np.zeros((H, W))
    for a in range(sub):
        for b in range(sub):
            u = (x + (a + 0.5) / sub) / (W - 1)                      # path_begin: x = px, y = H - py (row from the top)
            v = (H - row + (b + 0.5) / sub) / (H - 1)
            d = llc[None, None] + u[..., None] * hor + v[..., None] * ver - o
            t = -o[1] / d[..., 1]
            p = o + t[..., None] * d
            f += _form_factor(p[..., 0], p[..., 2])
    return ALBEDO * (f / (sub * sub))[..., None] * np.array(LE)[None, None, :]


def floor_rms(api, dev, cam, pred, W, H, spp, seeds, stratified):
    """RMS over pixels, channels and seeds of film - closed form, relative to the closed form's mean"""
    err = []
    for s in seeds:
        img, _ = dev.render_tile(cam, api.default_params(W, H, spp, max_depth=2, seed=s, nee=True, stratified=stratified))
        err.append(np.mean((img.astype(np.float64) - pred) ** 2))
    return float(np.sqrt(np.mean(err)) / pred.mean())


def cornell_ratio(api, dev, cam, W, H, nee):
    """-> (RMS default, RMS stratified) at 16 spp over 8 seeds against the mean of both samplers' 1024-spp films of another seed"""
    ref = np.zeros((H, W, 3))
    for strat in (False, True):
        img, _ = dev.render_tile(cam, api.default_params(W, H, 1024, seed=77777, nee=nee, stratified=strat))
        ref += 0.5 * img.astype(np.float64)
    rms = {}
    for strat in (False, True):
        err = [np.mean((dev.render_tile(cam, api.default_params(W, H, 16, seed=500 + s, nee=nee, stratified=strat))[0].astype(np.float64) - ref) ** 2)
               for s in range(8)]
        rms[strat] = float(np.sqrt(np.mean(err)))
    return rms[False], rms[True]


def test_report_the_error_ratio_on_cornell_box(cornell):
    """Reported, not asserted (DESIGN.md 4.9 quotes it): deep indirect light is where padding helps least."""
    api, hs, dev = cornell
    W = H = 64
    for nee in (False, True):
        a, b = cornell_ratio(api, dev, hs.camera(W, H), W, H, nee)
        _report(f"cornell_box 64x64 16 spp nee={nee}: RMS vs 2048-spp mean of both samplers: default {a:.5f}, stratified {b:.5f}, r = {b / a:.3f}")


def test_stratified_lowers_the_error_under_a_rect_light(built, tmp_path):
    """The floor of tests/test_gpu_nee.py (closed form albedo Le F: no render is its own yardstick), nee, max_depth 2, 64 x 64, seeds 0..7.
    Bound: half the measured gain, r <= 1 - (1 - R_MEASURED) / 2, which must lie at least three seed-group spreads above R_MEASURED."""
    from hobbyraytracer_amd import api
    bound = 1.0 - (1.0 - R_MEASURED) / 2.0                       # 0.6241
    assert bound >= R_MEASURED + 3.0 * R_SPREAD                  # (else the bound would be widened to that)
    hs = _scene(tmp_path, "floor", FLOOR_YAML)
    W = H = 64
    cam = hs.camera(W, H)
    pred = floor_prediction(cam, W, H)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        r = {}
        for spp in (4, 16, 64):
            a = floor_rms(api, dev, cam, pred, W, H, spp, range(8), False)
            b = floor_rms(api, dev, cam, pred, W, H, spp, range(8), True)
            r[spp] = b / a
            _report(f"floor 64x64 nee max_depth 2, {spp} spp, seeds 0..7: relative RMS default {a:.5f}, stratified {b:.5f}, r = {r[spp]:.3f}")
        assert r[16] <= bound, (r, bound)
    finally:
        dev.close()
