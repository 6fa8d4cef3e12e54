"""The float64 pins of tests/test_f64_pins.py on the HIP kernels: the renders on all three paths (per-round wavefront kernels,
k_wf_tail, the megakernel), the RNG keying of tiles, stripes and progressive passes, and the medium free path through
hrt_closest_hit."""
import numpy as np
import pytest

from tests import f64_cases as C
from tests import f64_reference as F

pytestmark = pytest.mark.gpu

PATHS = ["wavefront-rounds", "wavefront-tail", "megakernel"]


def _params(W, H, path, samples=1, thin=False):
    from hobbyraytracer_amd import api
    return api.default_params(W, H, samples, seed=C.SEED, thin_lens=thin, megakernel=(path == "megakernel"))


def _device(hs, path, monkeypatch):
    from hobbyraytracer_amd import api
    monkeypatch.setenv("HRT_WF_TAIL_ROUND", "1000" if path == "wavefront-rounds" else "1")
    return api.DeviceScene(hs.flat_ptr, 0)


def test_numpy_philox_equals_the_device(built):
    from hobbyraytracer_amd import api
    r = np.random.default_rng(3)
    c = r.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    k = r.integers(0, 2 ** 32, (4096, 2), dtype=np.uint64).astype(np.uint32)
    c[0], k[0] = [C.U0_PIXEL, 0, 0, F.RNG_MEDIUM], [C.SEED_LO, C.SEED_HI]
    got = api.math_probe(5, c.view(np.float32).ravel(), k.view(np.float32).ravel()).view(np.uint32).reshape(-1, 4)
    want = np.stack(F.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1]), axis=1)
    assert np.array_equal(got, want)
    assert got[0, 0] < 256


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", sorted(C.BG_CASES))
def test_background_texel_of_every_pixel(built, tmp_path, case, path, monkeypatch):
    cs = C.BG_CASES[case]
    hs = C.background_scene(tmp_path, cs)
    W, H = cs["W"], cs["H"]
    film, _ = _device(hs, path, monkeypatch).render_tile(hs.camera(W, H), _params(W, H, path, thin=cs.get("thin", False)))
    print(f"{case} {path}: ambiguous fraction {C.check_background(film, cs, (0, 0, W, H), 0):.5f}")


@pytest.mark.parametrize("path", PATHS)
def test_background_tile_with_an_offset(built, tmp_path, path, monkeypatch):
    cs = C.BG_CASES["odd_257x129"]
    hs = C.background_scene(tmp_path, cs)
    rect = (37, 21, 64, 40)
    film, _ = _device(hs, path, monkeypatch).render_tile(hs.camera(cs["W"], cs["H"]), _params(cs["W"], cs["H"], path), rect)
    C.check_background(film, cs, rect, 0)


@pytest.mark.parametrize("path", PATHS)
def test_background_one_stripe(built, tmp_path, path, monkeypatch):
    """Rank 1 of 3 of render_stripes (blocks of 4 rows): each row keyed by its global index."""
    from hobbyraytracer_amd import api
    cs = C.BG_CASES["odd_257x129"]
    hs = C.background_scene(tmp_path, cs)
    W, H = cs["W"], cs["H"]
    film, _ = _device(hs, path, monkeypatch).render_stripes(hs.camera(W, H), _params(W, H, path), 4, 1, 3)
    C.check_background(film, cs, (0, 0, W, film.shape[0]), 0, rows=api.stripe_row_indices(H, 4, 1, 3))


@pytest.mark.parametrize("path", ["wavefront-rounds", "wavefront-tail"])
def test_background_progressive_pass_at_sample_5(built, tmp_path, path, monkeypatch):
    """One render_stripes_accumulate pass over sample 5 of 8 (rank 1 of 3): the sums hold exactly sample 5's texel, keyed by the
    global pixel and sample index.  (The megakernel renders whole films only.)"""
    from hobbyraytracer_amd import api
    cs = C.BG_CASES["seam_minus_x"]
    hs = C.background_scene(tmp_path, cs)
    W, H = cs["W"], cs["H"]
    rows = api.stripe_row_indices(H, 4, 1, 3)
    acc = np.zeros((len(rows), W, 3), np.float32)
    _device(hs, path, monkeypatch).render_stripes_accumulate(hs.camera(W, H), _params(W, H, path, samples=8), 4, 1, 3, acc, 5, 1)
    C.check_background(acc, cs, (0, 0, W, len(rows)), 5, rows=rows)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", ["rect", "sphere"])
@pytest.mark.parametrize("size", C.IMAGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_texel_on_an_emitter(built, tmp_path, size, shape, path, monkeypatch):
    hs = C.image_scene(tmp_path, size, shape)
    cam = C.EMIT_CAM if shape == "rect" else C.SPHERE_CAM
    film, _ = _device(hs, path, monkeypatch).render_tile(hs.camera(cam["W"], cam["H"]), _params(cam["W"], cam["H"], path))
    print(f"image {size} {shape} {path}: ambiguous fraction {C.check_image(film, size, shape):.5f}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", ["rect", "sphere"])
def test_checkered_sign_on_an_emitter(built, tmp_path, shape, path, monkeypatch):
    hs = C.checker_scene(tmp_path, shape)
    cam = C.CHECK_CAM if shape == "rect" else C.CHECK_SPHERE_CAM
    film, _ = _device(hs, path, monkeypatch).render_tile(hs.camera(cam["W"], cam["H"]), _params(cam["W"], cam["H"], path))
    print(f"checker {shape} {path}: ambiguous fraction {C.check_checker(film, shape):.5f}")


@pytest.mark.parametrize("density", [0.7, 3.0])
@pytest.mark.parametrize("kind", ["box", "sphere"])
def test_medium_free_path(built, tmp_path, kind, density):
    from hobbyraytracer_amd import api
    hs = C.medium_scene(tmp_path, kind, density)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    p = api.default_params(8, 8, 1, seed=C.SEED)
    report = []
    for name, (o, d, t_min, t_max) in C.medium_ray_sets(kind).items():
        hits = dev.closest_hit(p, o, d, t_min, t_max, C.PIXEL0)
        try:
            frac, _, amb = C.check_medium(hits, kind, density, o, d, t_min, t_max, C.medium_u(len(o)))
        except AssertionError as e:
            raise AssertionError(f"ray set {name}: {e}") from None
        report.append(f"{name} {frac:.4f}")
        if name == "outside":
            D, n = C.ks_free_path(hits, kind, density, o, d, amb)
            report.append(f"KS D={D:.4f} n={n} D*sqrt(n)={D * np.sqrt(n):.3f}")
    print(f"medium {kind} rho={density} gpu: " + ", ".join(report))


def test_medium_thin_box_and_u0(built, tmp_path):
    from hobbyraytracer_amd import api
    C.check_thin_and_u0(lambda hs: api.DeviceScene(hs.flat_ptr, 0), tmp_path, api.default_params(8, 8, 1, seed=C.SEED))
