"""Float64 pins of the camera, the miss branch, the image / environment / checkered textures and ConstantMedium's free path,
run on the CPU oracle and on the device code compiled for the CPU (tests/tools/flatcpu_py.FlatCpu).  The expected values come
from tests/f64_reference.py, which shares no code with either; the parity tests cannot see a misreading of the reference that
both sides share, these can.  tests/test_gpu_f64_pins.py runs the same cases on the HIP kernels."""
import numpy as np
import pytest

from tests import f64_cases as C
from tests import f64_reference as F

IMPLS = ["oracle", "flatcpu"]


def _impl(name, hs):
    if name == "oracle":
        from oracle import oracle_py
        return oracle_py.World(hs.flat_ptr)
    from tests.tools.flatcpu_py import FlatCpu
    return FlatCpu(hs.flat_ptr)


def _params(W, H, samples=1, thin=False):
    from hobbyraytracer_amd import api
    return api.default_params(W, H, samples, seed=C.SEED, thin_lens=thin)


def test_numpy_philox_known_answers():
    """The float64 reference's Philox is the published one (Random123 kat_vectors, as in test_philox_known_answers)."""
    def run(c, k):
        return [int(x) for x in F.philox4x32_10(*c, *k)]
    assert run([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert run([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert run([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_numpy_philox_equals_the_oracle_restatement(built):
    from oracle import oracle_py
    r = np.random.default_rng(3)
    c = r.integers(0, 2 ** 32, (500, 4), dtype=np.uint64).astype(np.uint32)
    k = r.integers(0, 2 ** 32, (500, 2), dtype=np.uint64).astype(np.uint32)
    got = oracle_py.math_probe(5, c.view(np.float32).ravel(), k.view(np.float32).ravel()).view(np.uint32).reshape(-1, 4)
    want = np.stack(F.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1]), axis=1)
    assert np.array_equal(got, want)


def test_u0_counter_is_the_first_one_under_the_seed():
    """C.U0_PIXEL is found by a search over 2^24 pixel indices: the ray keyed by it draws u = 0 for the medium (ln 0 = -inf)."""
    x = F.draw(C.SEED_LO, C.SEED_HI, np.uint64(C.U0_PIXEL), 0, 0, F.RNG_MEDIUM, 0)[0]
    assert int(x) < 256 and F.u01(x) == 0.0
    found = []
    for base in range(0, 1 << 24, 1 << 21):
        pix = np.arange(base, base + (1 << 21), dtype=np.uint64)
        found += pix[F.draw(C.SEED_LO, C.SEED_HI, pix, 0, 0, F.RNG_MEDIUM, 0)[0] < 256].tolist()
    assert found and found[0] == C.U0_PIXEL


# ------------------------------------------------------------------ camera + miss branch + EnvironmentMap
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", sorted(C.BG_CASES))
def test_background_texel_of_every_pixel(built, tmp_path, case, impl):
    """Primary ray (Q-10 row convention, W-1 / H-1, jitter counter) and the miss lookup: each pixel must read the float64
    texel.  One sample per pixel, so the film value is that texel."""
    cs = C.BG_CASES[case]
    hs = C.background_scene(tmp_path, cs)
    W, H = cs["W"], cs["H"]
    film, _ = _impl(impl, hs).render_tile(hs.camera(W, H), _params(W, H, thin=cs.get("thin", False)))
    frac = C.check_background(film, cs, (0, 0, W, H), 0)
    print(f"{case} {impl}: ambiguous fraction {frac:.5f}")


@pytest.mark.parametrize("impl", IMPLS)
def test_background_tile_with_an_offset(built, tmp_path, impl):
    """A tile away from the film's origin: the jitter is keyed by the GLOBAL pixel index."""
    cs = C.BG_CASES["odd_257x129"]
    hs = C.background_scene(tmp_path, cs)
    rect = (37, 21, 64, 40)
    film, _ = _impl(impl, hs).render_tile(hs.camera(cs["W"], cs["H"]), _params(cs["W"], cs["H"]), rect)
    C.check_background(film, cs, rect, 0)


@pytest.mark.parametrize("impl", IMPLS)
def test_background_second_sample(built, tmp_path, impl):
    """Two samples: the film is the mean of samples 0 and 1, each keyed by its own sample index."""
    cs = C.BG_CASES["seam_minus_x"]
    hs = C.background_scene(tmp_path, cs)
    W, H = cs["W"], cs["H"]
    film, _ = _impl(impl, hs).render_tile(hs.camera(W, H), _params(W, H, samples=2))
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    vals, amb = [], np.zeros((H, W), bool)
    for s in (0, 1):
        _, d = F.primary_rays(C.f64_camera(cs), W, H, px, py, s, C.SEED_LO, C.SEED_HI)
        u, v = F.miss_uv(d)
        du, dv = F.miss_uv_delta(d)
        i, _, _, ai = F.band_wrap(lambda x: F.env_index(x, cs["env"][0]), u, du)
        j, _, _, aj = F.band(lambda x: F.env_index(x, cs["env"][1]), v, dv)
        vals.append(np.stack([i, j, np.full_like(i, C.ENV_TAG)], -1))
        amb |= ai | aj
    assert amb.mean() < C.MAX_AMBIGUOUS
    want = ((C._LDR[vals[0]] + C._LDR[vals[1]]) / 2)
    assert np.allclose(film[~amb], want[~amb], rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------ ImageTexture, rect and sphere UVs, CheckeredTexture
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("shape", ["rect", "sphere"])
@pytest.mark.parametrize("size", C.IMAGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_texel_on_an_emitter(built, tmp_path, size, shape, impl):
    """DiffuseLight with an image albedo fills the view: each pixel is 2 * texel / 255 of the float64 texel (int(u W), the v
    flip, the clamps), or the background."""
    hs = C.image_scene(tmp_path, size, shape)
    cam = C.EMIT_CAM if shape == "rect" else C.SPHERE_CAM
    film, _ = _impl(impl, hs).render_tile(hs.camera(cam["W"], cam["H"]), _params(cam["W"], cam["H"]))
    frac = C.check_image(film, size, shape)
    print(f"image {size} {shape} {impl}: ambiguous fraction {frac:.5f}")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("shape", ["rect", "sphere"])
def test_checkered_sign_on_an_emitter(built, tmp_path, shape, impl):
    hs = C.checker_scene(tmp_path, shape)
    cam = C.CHECK_CAM if shape == "rect" else C.CHECK_SPHERE_CAM
    film, _ = _impl(impl, hs).render_tile(hs.camera(cam["W"], cam["H"]), _params(cam["W"], cam["H"]))
    frac = C.check_checker(film, shape)
    print(f"checker {shape} {impl}: ambiguous fraction {frac:.5f}")


# ------------------------------------------------------------------ ConstantMedium
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("density", [0.7, 3.0])
@pytest.mark.parametrize("kind", ["box", "sphere"])
def test_medium_free_path(built, tmp_path, kind, density, impl):
    hs = C.medium_scene(tmp_path, kind, density)
    world = _impl(impl, hs)
    p = _params(8, 8)
    report = []
    for name, (o, d, t_min, t_max) in C.medium_ray_sets(kind).items():
        hits = world.closest_hit(p, o, d, t_min, t_max, C.PIXEL0)
        u = C.medium_u(len(o))
        try:
            frac, t1, amb = C.check_medium(hits, kind, density, o, d, t_min, t_max, u)
        except AssertionError as e:
            raise AssertionError(f"ray set {name}: {e}") from None
        report.append(f"{name} {frac:.4f}")
        if name == "outside":
            D, n = C.ks_free_path(hits, kind, density, o, d, amb)
            report.append(f"KS D={D:.4f} n={n} D*sqrt(n)={D * np.sqrt(n):.3f}")
    print(f"medium {kind} rho={density} {impl}: " + ", ".join(report))


@pytest.mark.parametrize("impl", IMPLS)
def test_medium_thin_box_and_u0(built, tmp_path, impl):
    C.check_thin_and_u0(lambda hs: _impl(impl, hs), tmp_path, _params(8, 8))
