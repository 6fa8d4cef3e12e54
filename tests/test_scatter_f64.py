"""Float64 pins of Material::scatter and of the rayColour loop on the CPU.

Layer A: oracle_py.World.scatter, ray by ray, against tests/f64_scatter.py with the same Philox counters: 20 000 rays per case
at one big rect, one sphere or one ConstantMedium box, directions un-normalised (scaled by 1.7) as the path tracer's are.
Layer B: depth-limited films of tests/f64_scatter_cases.py on the oracle and on the device code compiled for the CPU
(tests/tools/flatcpu_py.FlatCpu); tests/test_gpu_scatter_f64.py runs the same films on the HIP kernels.

The expected values share no code with hrt_glm.h / hrt_rng.h / hrt_device.h, which the oracle includes: a misreading of
material.h, of glm's sphericalRand / ballRand / reflect / refract or of the counter keying that moves the oracle and the
kernels together shows here.  Tolerances: S.SD_ATOL (5e-6) on the components of a direction built from sphericalRand and on
attenuations, S.MIRROR_ATOL (3e-7) on a smooth metal's direction; a ray whose decision margin is below F.EPS must equal one of
the two float64 outcomes, and fewer than 2 % of a case's rays may be such."""
import numpy as np
import pytest

from tests import f64_cases as C
from tests import f64_reference as F
from tests import f64_scatter as S
from tests import f64_scatter_cases as SC

IMPLS = ["oracle", "flatcpu"]
N = 20000
PIXEL0 = 5000
QUIRKS = ["reference", "fixed"]


def _impl(name, hs):
    if name == "oracle":
        from oracle import oracle_py
        return oracle_py.World(hs.flat_ptr)
    from tests.tools.flatcpu_py import FlatCpu
    return FlatCpu(hs.flat_ptr)


def _params(quirks="reference", max_depth=50):
    from hobbyraytracer_amd import api
    q = api.QUIRKS_REFERENCE if quirks == "reference" else api.QUIRKS_FIXED
    return api.default_params(SC.W, SC.H, 1, quirks=q, seed=C.SEED, max_depth=max_depth)


# ------------------------------------------------------------------ layer A
RECT = dict(shape="xy_rect", a=(-50.0, 50.0), b=(-50.0, 50.0), k=0.0)
BALL = dict(shape="sphere", center=(0.0, 0.0, 0.0), radius=1.0)


def _scene(tmp_path, name, materials, obj, textures=""):
    from hobbyraytracer_amd import api
    y = C._camera_yaml(8, 8, (0, 0, 9), (0, 0, 0), (0, 1, 0), 40, 0.0, 1.0, "[0, 0, 0]")
    y += textures + "materials:\n" + materials + "objects:\n" + obj
    p = tmp_path / f"{name}.yaml"
    p.write_text(y)
    return api.HostScene(str(p), str(tmp_path))


_RECT_YAML = "  - type: xy_rect\n    x: [-50, 50]\n    y: [-50, 50]\n    k: 0\n    material: m\n"
_BALL_YAML = "  - type: sphere\n    center: [0, 0, 0]\n    radius: 1.0\n    material: m\n"


def rect_rays(theta_deg, from_above=True, seed=4):
    """N rays onto the big rect at one angle of incidence, origins spread over 10 x 10, directions of length 1.7."""
    r = np.random.default_rng(seed)
    th = np.radians(theta_deg)
    d = np.array([np.sin(th), 0.0, -np.cos(th) if from_above else np.cos(th)]) * 1.7
    o = np.stack([r.uniform(-5, 5, N), r.uniform(-5, 5, N), np.full(N, 2.0 if from_above else -2.0)], 1)
    return o.astype(np.float32), np.tile(d.astype(np.float32), (N, 1))


def ball_rays(seed=6):
    """N rays from a shell of radius 3 towards points inside the unit sphere (all hit it), directions of length 1.7."""
    r = np.random.default_rng(seed)
    v = r.normal(size=(N, 3))
    o = 3.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
    tgt = r.uniform(-0.55, 0.55, (N, 3))
    d = tgt - o
    return o.astype(np.float32), (1.7 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def f64_hit(ob, o, d):
    """The float64 hit record of every ray (all rays of a layer-A set hit their object well inside it)."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    if ob["shape"] == "sphere":
        t, _, _ = F.sphere_roots(o, d, ob["center"], ob["radius"])
    else:
        t, _, inside = F.rect_hit(o, d, 2, *ob["a"], *ob["b"], ob["k"])
        assert inside.all()
    assert np.all(t > 0.01)
    return S.hit_record(ob, o, d, t)


def _key(n=N, pixel0=PIXEL0):
    return dict(seed_lo=C.SEED_LO, seed_hi=C.SEED_HI, pixel=np.arange(pixel0, pixel0 + n, dtype=np.uint64), sample=0, bounce=0)


def _agrees(got, s, sd_atol):
    sd, att, flag = got
    ok = flag == s["scattered"].astype(np.int32)
    ok &= (np.abs(att - s["attenuation"]) <= S.SD_ATOL).all(-1)
    ok &= ~s["scattered"] | (np.abs(sd - s["sd"]) <= sd_atol).all(-1)
    return ok


def check_scatter(got, mat, rec, d, key=None, sd_atol=S.SD_ATOL, alt_mat=None, extra_amb=None, label=""):
    """got = (sd, attenuation, flag) of the implementation.  Every unambiguous ray equals the float64 scatter; an ambiguous one
    equals it or the outcome with its ambiguous decisions taken the other way.  -> (the float64 scatter, ambiguous mask)."""
    key = key or _key(len(d))
    s = S.scatter(mat, rec, d, key)
    masks, amb = S.ambiguous(s["margins"])
    alt = S.scatter(alt_mat or mat, rec, d, key, flip=masks)
    if extra_amb is not None:
        amb = amb | extra_amb
    frac = float(np.mean(amb))
    print(f"{label}: ambiguous share {frac:.5f}")
    assert frac < C.MAX_AMBIGUOUS, f"ambiguity band too wide: {frac:.4f}"
    ok = _agrees(got, s, sd_atol)
    bad = ~amb & ~ok
    assert not bad.any(), _first(bad, got, s)
    bad = amb & ~(ok | _agrees(got, alt, sd_atol))
    assert not bad.any(), "in the band: " + _first(bad, got, s)
    return s, amb


def _first(bad, got, s):
    i = int(np.nonzero(bad)[0][0])
    return (f"{int(bad.sum())} rays differ from the float64 scatter, first: ray {i} got flag {got[2][i]} sd {got[0][i]} att {got[1][i]}, "
            f"expected {int(s['scattered'][i])} {s['sd'][i]} {s['attenuation'][i]}")


def _run(hs, quirks, o, d):
    from oracle import oracle_py
    sd, att, flag, hits = oracle_py.World(hs.flat_ptr).scatter(_params(quirks), o, d, PIXEL0)
    return (sd, att, flag), hits


@pytest.mark.parametrize("quirks", QUIRKS)
@pytest.mark.parametrize("shape", ["rect", "sphere"])
def test_lambertian_ray_by_ray(built, tmp_path, shape, quirks):
    """material.h:137-153: sd = n + sphericalRand(1) from words x, y of (pixel, 0, 0, RNG_SCATTER); |sd - n| = 1."""
    mats = "  - name: m\n    type: lambertian\n    albedo: [0.8, 0.4, 0.3]\n"
    ob, (o, d) = (RECT, rect_rays(35.0)) if shape == "rect" else (BALL, ball_rays())
    hs = _scene(tmp_path, "lam", mats, _RECT_YAML if shape == "rect" else _BALL_YAML)
    got, hits = _run(hs, quirks, o, d)
    rec = f64_hit(ob, o, d)
    assert np.abs(hits["normal"] - rec["normal"]).max() < S.SD_ATOL and (hits["front_face"] == 1).all()
    s, _ = check_scatter(got, SC.lambertian(np.float32([0.8, 0.4, 0.3])), rec, d, label=f"lambertian {shape}")
    assert (got[2] == 1).all()
    np.testing.assert_allclose(np.linalg.norm(got[0].astype(np.float64) - rec["normal"], axis=1), 1.0, atol=S.SD_ATOL)


@pytest.mark.parametrize("quirks", QUIRKS)
def test_uvtest_attenuation_is_the_normal(built, tmp_path, quirks):
    hs = _scene(tmp_path, "uv", "  - name: m\n    type: uv_test\n", _BALL_YAML)
    o, d = ball_rays()
    got, _ = _run(hs, quirks, o, d)
    rec = f64_hit(BALL, o, d)
    check_scatter(got, dict(kind=S.UVTEST), rec, d, label="uv_test")
    np.testing.assert_allclose(got[1], rec["normal"], atol=S.SD_ATOL)


@pytest.mark.parametrize("quirks", QUIRKS)
@pytest.mark.parametrize("theta", [0.0, 60.0, 85.0])
@pytest.mark.parametrize("rough", [0.3, 1.0, 2.5, -0.4])
def test_rough_metal_ray_by_ray(built, tmp_path, rough, theta, quirks):
    """material.h:166-177: sd = reflect + min(|r|, 1) sphericalRand + epsilon; scattered = dot(sd, n) > 0."""
    mats = f"  - name: m\n    type: metal\n    albedo: [0.9, 0.6, 0.3]\n    roughness: {rough}\n"
    hs = _scene(tmp_path, "met", mats, _RECT_YAML)
    o, d = rect_rays(theta)
    got, _ = _run(hs, quirks, o, d)
    rec = f64_hit(RECT, o, d)
    s, amb = check_scatter(got, SC.metal(np.float32(rough), np.float32([0.9, 0.6, 0.3])), rec, d, label=f"metal {rough} at {theta}")
    sd = got[0].astype(np.float64)
    assert np.array_equal((got[2] == 1)[~amb], (sd[:, 2] > 0)[~amb] & s["scattered"][~amb])
    rho = min(abs(rough), 1.0)
    di = d[0].astype(np.float64) / np.linalg.norm(d[0].astype(np.float64))
    centre = di - 2 * di[2] * np.array([0, 0, 1.0]) + S.EPS_F32
    on = got[2] == 1
    np.testing.assert_allclose(np.linalg.norm(sd[on] - centre, axis=1), rho, atol=2 * S.SD_ATOL)      # the clamp and the fabs
    if theta == 85.0 and rough == 1.0:
        assert 0.2 < (got[2] == 0).mean() < 0.8, "at 85 degrees with rho = 1 both flags must occur"
    if theta == 0.0 and rho < 1.0:
        assert (got[2] == 1).all()


@pytest.mark.parametrize("quirks", QUIRKS)
def test_smooth_metal_keeps_its_tolerance(built, tmp_path, quirks):
    mats = "  - name: m\n    type: metal\n    albedo: [0.9, 0.6, 0.3]\n    roughness: 0.0\n"
    hs = _scene(tmp_path, "mir", mats, _RECT_YAML)
    for theta in (0.0, 60.0, 85.0):
        o, d = rect_rays(theta)
        got, _ = _run(hs, quirks, o, d)
        check_scatter(got, SC.metal(0.0, np.float32([0.9, 0.6, 0.3])), f64_hit(RECT, o, d), d, sd_atol=S.MIRROR_ATOL,
                      label=f"smooth metal at {theta}")


@pytest.mark.parametrize("quirks", QUIRKS)
def test_smooth_metal_adds_epsilon_exactly(built, tmp_path, quirks):
    """material.h:173's + vec3(epsilon) is smaller than MIRROR_ATOL, so it gets a case where fp32 is exact: straight down along
    (0, 0, -2) every operation of normalize and reflect is exact (4, 2, 1 / 2), and sd must be (eps, eps, 1 + eps) to the bit."""
    mats = "  - name: m\n    type: metal\n    albedo: [0.9, 0.6, 0.3]\n    roughness: 0.0\n"
    hs = _scene(tmp_path, "eps", mats, _RECT_YAML)
    o, _ = rect_rays(0.0)
    d = np.tile(np.float32([0.0, 0.0, -2.0]), (N, 1))
    got, _ = _run(hs, quirks, o, d)
    s = S.scatter(SC.metal(0.0, np.float32([0.9, 0.6, 0.3])), f64_hit(RECT, o, d), d, _key())
    assert np.array_equal(s["sd"], np.tile([S.EPS_F32, S.EPS_F32, 1.0 + S.EPS_F32], (N, 1)))
    assert np.array_equal(got[0].astype(np.float64), s["sd"]) and (got[2] == 1).all()


ROUGH_BYTES = (60, 60, 41)        # ImageTexture (texture.cpp:34, 70-73: stbi_load and byte / 255): length 0.3696


@pytest.mark.parametrize("quirks", QUIRKS)
def test_metal_roughness_from_an_image_is_the_length_of_its_rgb(built, tmp_path, quirks):
    """MatScalar::valueAt (material.h:43-54) of a texture: glm::length(rgb).  A constant-colour image of ROUGH_BYTES."""
    from hobbyraytracer_amd import api
    api.write_image(str(tmp_path / "rough.png"), np.tile(np.uint8(ROUGH_BYTES), (4, 4, 1)))
    rho = float(np.sqrt(sum((b / 255.0) ** 2 for b in ROUGH_BYTES)))
    assert abs(rho - 0.37) < 1e-3
    tex = "textures:\n  - name: rough\n    type: image\n    path: rough.png\n"
    mats = "  - name: m\n    type: metal\n    albedo: [1, 1, 1]\n    roughness: rough\n"
    hs = _scene(tmp_path, "mtex", mats, _RECT_YAML, tex)
    o, d = rect_rays(60.0)
    got, _ = _run(hs, quirks, o, d)
    check_scatter(got, SC.metal(rho), f64_hit(RECT, o, d), d, label="metal, roughness from an image")
    on = got[2] == 1
    di = d[0].astype(np.float64) / np.linalg.norm(d[0].astype(np.float64))
    centre = di - 2 * di[2] * np.array([0, 0, 1.0]) + S.EPS_F32
    np.testing.assert_allclose(np.linalg.norm(got[0][on] - centre, axis=1), rho, atol=2 * S.SD_ATOL)


@pytest.mark.parametrize("quirks", QUIRKS)
@pytest.mark.parametrize("from_above", [True, False], ids=["entering", "leaving"])
@pytest.mark.parametrize("rough", [0.0, 0.25])
def test_dielectric_ray_by_ray(built, tmp_path, rough, from_above, quirks):
    """material.h:204-241: per ray reflected exactly when Schlick (of the refraction RATIO) > the coin u01d(z, w), always beyond
    the critical angle; reflect / refract; + r sphericalRand(x, y)."""
    mats = f"  - name: m\n    type: dielectric\n    ior: 1.5\n    roughness: {rough}\n"
    hs = _scene(tmp_path, "die", mats, _RECT_YAML)
    mat = SC.glass(np.float32(rough))
    for theta in (0.0, 30.0, 40.0, 60.0, 80.0):
        o, d = rect_rays(theta, from_above)
        got, hits = _run(hs, quirks, o, d)
        rec = f64_hit(RECT, o, d)
        assert (hits["front_face"] == (1 if from_above else 0)).all() and rec["front_face"].all() == from_above
        s, amb = check_scatter(got, mat, rec, d, label=f"dielectric {rough} {'in' if from_above else 'out'} at {theta}")
        assert (got[2] == 1).all() and (got[1] == 1).all()
        ratio = 1 / 1.5 if from_above else 1.5
        tir = ratio * np.sin(np.radians(theta)) > 1.0
        assert s["tir"].all() == tir and s["tir"].any() == tir
        assert np.array_equal(s["reflected"], s["tir"] | (s["schlick"] > s["coin"]))
        if rough == 0.0:           # the side the ray leaves on is the choice itself
            side = -1.0 if from_above else 1.0
            reflected = np.sign(got[0][:, 2]) != side
            assert np.array_equal(reflected[~amb], s["reflected"][~amb])
            assert reflected.all() or not tir
            if not tir and theta > 0:
                assert reflected.any() and (~reflected).any()
        if theta == 60.0 and from_above and quirks == "reference":
            # the test's power: with the roles of the words (x, y) and (z, w) exchanged in the reference, the same rays fail
            swapped = S.scatter(mat, rec, d, _key(), words=("z", "w", "x", "y"))
            assert (~_agrees(got, swapped, S.SD_ATOL)).mean() > (0.5 if rough else 0.05)
            coin_swapped = S.scatter(mat, rec, d, _key(), words=("x", "y", "w", "z"))
            assert (~_agrees(got, coin_swapped, S.SD_ATOL)).mean() > 0.03


@pytest.mark.parametrize("quirks", QUIRKS)
def test_isotropic_ray_by_ray(built, tmp_path, quirks):
    """material.h:79-85 inside a ConstantMedium box: sd = ballRand(1) with one Philox call per attempt (RNG_BALL, aux = attempt);
    attenuation = the medium's colour; always scattered.  Which rays hit the medium is the float64 free path's say."""
    density = 3.0
    hs = C.medium_scene(tmp_path, "box", density)
    o, d, t_min, t_max = C.medium_ray_sets("box")["outside"]
    got, hits = _run(hs, quirks, o, d)
    key = _key(len(o))
    t, _, amb_hit = F.medium_free_path("box", C.MEDIUM_BOX, np.float64(np.float32(density)), o.astype(np.float64), d.astype(np.float64),
                                       t_min, t_max, C.medium_u(len(o), PIXEL0))
    want_hit = np.isfinite(t)
    assert np.array_equal((got[2] >= 0)[~amb_hit], want_hit[~amb_hit]) and amb_hit.mean() < C.MAX_AMBIGUOUS
    sel = want_hit & (got[2] >= 0)
    assert sel.sum() > 5000
    sub = dict(key, pixel=key["pixel"][sel])
    p = o[sel].astype(np.float64) + t[sel, None] * d[sel].astype(np.float64)
    rec = dict(p=p, normal=np.tile([1.0, 0.0, 0.0], (len(p), 1)), front_face=np.ones(len(p), bool))
    mat = dict(kind=S.ISOTROPIC, albedo=np.float32([0.9, 0.4, 0.4]))
    s, _ = check_scatter(tuple(g[sel] for g in got), mat, rec, d[sel], key=sub, label="isotropic")
    assert (got[2][sel] == 1).all()
    assert s["attempts"].max() >= 3 and (s["attempts"] == 1).mean() < 0.6, "the rays must include rejected attempts"
    assert (np.linalg.norm(got[0][sel].astype(np.float64), axis=1) <= 1 + 1e-6).all()


@pytest.mark.parametrize("quirks", QUIRKS)
def test_diffuse_light_does_not_scatter(built, tmp_path, quirks):
    mats = "  - name: m\n    type: diffuse_light\n    albedo: [0.9, 0.5, 0.2]\n    strength: 3.5\n"
    hs = _scene(tmp_path, "lamp", mats, _RECT_YAML)
    for above in (True, False):
        o, d = rect_rays(30.0, above)
        got, _ = _run(hs, quirks, o, d)
        check_scatter(got, SC.light((0.9, 0.5, 0.2), 3.5), f64_hit(RECT, o, d), d, label="diffuse light")
        assert (got[2] == 0).all() and (got[1] == 0).all()


@pytest.mark.parametrize("quirks", QUIRKS)
def test_pbr_mix_chooses_by_the_length_of_the_mix_texel(built, tmp_path, quirks):
    """material.cpp:18-28 with the two-texel mix image of the cases module: u < 0.5 (x < 0) scatters as a Lambertian, the right
    half as a Metal of roughness PBR_RHO."""
    from hobbyraytracer_amd import api
    api.write_image(str(tmp_path / "mix.png"), SC.MIX_BYTES)
    tex = "textures:\n  - name: mix\n    type: image\n    path: mix.png\n"
    mats = (f"  - name: m\n    type: pbr\n    albedo: [1, 1, 1]\n    metalness: 0.0\n    roughness: {SC.PBR_RHO}\n"
            "  - name: carrier\n    type: lambertian\n    albedo: mix\n")
    obj = _RECT_YAML + "  - type: sphere\n    center: [0, 0, -900]\n    radius: 0.5\n    material: carrier\n"
    hs = _scene(tmp_path, "pbr", mats, obj, tex)
    SC.point_pbr_mix_at_image(hs)
    o, d = rect_rays(60.0)
    o[:, 0] -= np.float32(2.0 * np.tan(np.radians(60.0)))             # the hit points straddle x = 0, the texels' border
    got, _ = _run(hs, quirks, o, d)
    rec = f64_hit(RECT, o, d)
    resolve = SC.pbr_mix(RECT)
    mat, texel_amb = resolve(rec, False)
    alt, _ = resolve(rec, True)
    assert SC.MIX_LEN[0] < 0.25 and SC.MIX_LEN[1] > 0.75
    s, amb = check_scatter(got, mat, rec, d, alt_mat=alt, extra_amb=texel_amb, label="pbr mix")
    left = rec["p"][:, 0] < 0
    assert left.mean() > 0.3 and (~left).mean() > 0.3
    sd = got[0].astype(np.float64)
    np.testing.assert_allclose(np.linalg.norm(sd[left & ~amb] - [0, 0, 1.0], axis=1), 1.0, atol=2 * S.SD_ATOL)      # n + sph
    assert (got[2][left & ~amb] == 1).all()
    as_metal = S.scatter(SC.metal(SC.PBR_RHO), rec, d, _key())
    assert _agrees(got, as_metal, S.SD_ATOL)[~left & ~amb].all() and not _agrees(got, as_metal, S.SD_ATOL)[left].any()


@pytest.mark.parametrize("quirks", QUIRKS)
def test_pbr_mix_of_exactly_one_half_is_diffuse(built, tmp_path, quirks):
    """material.cpp:20: length(mix) > 0.5f, strictly.  A solid mix colour (0.5, 0, 0) has length exactly 0.5 in fp32 (0.25 and its
    root are exact), so the PBR scatters as a Lambertian; the next float above 0.5 scatters as a Metal."""
    from hobbyraytracer_amd import api
    above = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    o, d = rect_rays(60.0)
    rec = f64_hit(RECT, o, d)
    for value, kind in ((0.5, S.LAMBERTIAN), (above, S.METAL)):
        tex = f"textures:\n  - name: half\n    type: solid\n    colour: [{value!r}, 0.0, 0.0]\n"
        mats = (f"  - name: m\n    type: pbr\n    albedo: [1, 1, 1]\n    metalness: 0.0\n    roughness: {SC.PBR_RHO}\n"
                "  - name: carrier\n    type: lambertian\n    albedo: half\n")
        obj = _RECT_YAML + "  - type: sphere\n    center: [0, 0, -900]\n    radius: 0.5\n    material: carrier\n"
        hs = _scene(tmp_path, f"half_{kind}", mats, obj, tex)
        SC.point_pbr_mix_at_image(hs, lambda t: t.kind == api.TEX_SOLID and t.c[0] == np.float32(value) and t.c[1] == 0.0)
        got, _ = _run(hs, quirks, o, d)
        check_scatter(got, dict(kind=kind, albedo=SC.WHITE, roughness=SC.PBR_RHO), rec, d, label=f"pbr, mix length {value!r}")


# ------------------------------------------------------------------ layer B
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", sorted(SC.CASES))
def test_depth_limited_film(built, tmp_path, case, impl):
    """main.cpp:38-79: result += atten * emitted, atten *= attenuation, the segment index in the RNG key, the cut at max_depth."""
    hs = SC.build_scene(tmp_path, case)
    film, _ = _impl(impl, hs).render_tile(hs.camera(SC.W, SC.H), _params(max_depth=SC.CASES[case]["max_depth"]))
    frac = SC.check_film(film, case)
    print(f"{case} {impl}: ambiguous share {frac:.5f}")
