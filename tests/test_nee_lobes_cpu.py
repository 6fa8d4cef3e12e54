"""Light sampling at rough metal and medium vertices (HRT_FLAG_NEE_LOBES) without a GPU: the lobe helpers of
hrt_device.h compiled for the host (tests/tools/nee_lobes_on_cpu.cpp) against numpy -- the density of material_scatter's Metal
scatter, its roots and their shares, the Isotropic scatter's density and length law, eligibility around HRT_NEE_RHO_MIN."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_ISOTROPIC, MAT_UVTEST = 0, 1, 2, 4, 6      # include/hrt.h
LOBE_NONE, LOBE_METAL, LOBE_MEDIUM = 0, 1, 2                                               # hrt_device.h
NN = np.array([0.0, 1.0, 0.0], np.float32)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("neelobes") / "libneelobescpu.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-shared", "-o", so,
                           os.path.join(HERE, "tools", "nee_lobes_on_cpu.cpp")])
    L = C.CDLL(so)
    L.nee_rho_min.restype = C.c_float
    L.lobe_m.argtypes = [F, F, C.c_float, F]
    L.nee_lobe_pdf_batch.argtypes = [F, C.c_int64, F, F]
    L.nee_vertex_pdf_batch.argtypes = [F, F, C.c_int64, F, F]
    L.scatter_lobe.argtypes = [C.c_int, C.c_float, F, F, F]
    L.nee_vertex_inv_acc_c.argtypes = [F, F]
    L.nee_vertex_inv_acc_c.restype = C.c_float
    L.nee_vertex_len_c.argtypes = [C.c_float, C.c_float, C.c_uint32]
    L.nee_vertex_len_c.restype = C.c_float
    L.nee_pick_root_c.argtypes = [C.c_float, C.c_float, C.c_uint32]
    L.nee_pick_root_c.restype = C.c_float
    for f in (L.nee_mis_bsdf_c, L.nee_mis_shadow_c):
        f.argtypes = [C.c_float, C.c_float]
        f.restype = C.c_float
    L.metal_scatter_dirs.argtypes = [F, F, C.c_float, C.c_uint32, C.c_int64, F]
    L.ball_scatter_dirs.argtypes = [C.c_uint32, C.c_int64, F]
    return L


def incidence(angle):
    """a direction arriving at the floor (normal +y) at `angle` from the normal, with a z component"""
    return np.array([np.sin(angle), -np.cos(angle), 0.3 * np.sin(angle)], np.float32)


def lobe(lib, rho, angle):
    m = np.zeros(3, np.float32)
    lib.lobe_m(incidence(angle), NN, rho, m)
    return m


def axis_frame(m):
    a = m.astype(np.float64)
    r = np.linalg.norm(a)
    a /= r
    b = np.cross(a, [1.0, 0.0, 0.0]); b /= np.linalg.norm(b)
    return a, b, r


def p_of_mu(lib, m, mu):
    """nee_lobe_pdf at cosine mu to the lobe's axis (the density depends on that angle alone)"""
    a, b, _ = axis_frame(m)
    s = np.sqrt(np.maximum(0.0, 1.0 - mu * mu))
    w = np.ascontiguousarray(mu[:, None] * a[None, :] + s[:, None] * b[None, :], np.float32)
    out = np.zeros((len(w), 3), np.float32)
    lib.nee_lobe_pdf_batch(m, len(w), w, out)
    return out[:, 0].astype(np.float64)


def mu_grid(m, k):
    """midpoints of k equal cells of [mu_lo, 1], mu_lo just below the edge of the cone the lobe fills (|m| > 1), and the cell width"""
    _, _, r = axis_frame(m)
    mu_lo = -1.0 if r <= 1.0 else max(-1.0, np.sqrt(max(0.0, 1.0 - 1.0 / (r * r))) - 1e-3 / (r * r))
    h = (1.0 - mu_lo) / k
    return mu_lo + (np.arange(k) + 0.5) * h, h


def rhos(lib):
    return [lib.nee_rho_min(), 0.05, 0.2, 0.8, 1.0]


@pytest.mark.parametrize("i_rho", range(5))
@pytest.mark.parametrize("angle", [0.1, 0.7, 1.3])
def test_metal_lobe_density_integrates_to_one(lib, i_rho, angle):
    # integral = 2 pi int p(mu) dmu over the cone (midpoint rule, 2 M cells as test_nee_cpu.test_pb_integrates_to_one; the same
    # tolerances: 2e-3 where |m| > 1 -- the integrable 1 / sqrt(D) edge -- and 2e-4 otherwise)
    rho = np.float32(rhos(lib)[i_rho])
    m = lobe(lib, rho, angle)
    mu, h = mu_grid(m, 2_000_000)
    total = 2.0 * np.pi * p_of_mu(lib, m, mu).sum() * h
    r = np.linalg.norm(m.astype(np.float64))
    print(f"rho {rho:.6f} angle {angle}: |m| {r:.6f}, integral {total:.6f}")
    assert abs(total - 1.0) < (2e-3 if r > 1.0 else 2e-4), total


@pytest.mark.parametrize("i_rho", range(5))
def test_metal_lobe_density_matches_the_scatter_histogram(lib, i_rho):
    # normalize(reflected + rho sphericalRand + eps) drawn with the product's own RNG, binned by mu = the cosine to the lobe's axis
    # over the cone; expected shares from nee_lobe_pdf alone.  40 bins and the significance of test_nee_cpu's histogram test.
    rho = np.float32(rhos(lib)[i_rho])
    angle = 0.7
    m = lobe(lib, rho, angle)
    a, _, r = axis_frame(m)
    n = 400_000
    out = np.zeros((n, 4), np.float32)
    lib.metal_scatter_dirs(incidence(angle), NN, rho, 12345, n, out)
    mu = out[:, :3].astype(np.float64) @ a
    grid, h = mu_grid(m, 400_000)
    lo = grid[0] - 0.5 * h
    edges = np.linspace(lo, 1.0, 41)
    hist = np.histogram(np.clip(mu, lo, 1.0), edges)[0]
    dens = 2.0 * np.pi * p_of_mu(lib, m, grid) * h
    expect = np.array([dens[(grid >= e0) & (grid < e1)].sum() for e0, e1 in zip(edges[:-1], edges[1:])]) * n
    keep = expect > 20.0
    assert hist[~keep].sum() <= max(40, 3 * expect[~keep].sum())
    chi2 = (((hist[keep] - expect[keep]) ** 2) / expect[keep]).sum()
    dof = keep.sum() - 1
    print(f"rho {rho:.6f}: chi2 {chi2:.1f}, dof {dof}")
    assert chi2 < dof + 6.0 * np.sqrt(2.0 * dof), (chi2, dof)
    # the lengths the scatter gave lie between the lobe's two roots times rho
    assert (out[:, 3] <= rho * (r + 1.0) * (1 + 1e-5)).all() and (out[:, 3] >= rho * (r - 1.0) * (1 - 1e-5) - 1e-6).all()


def test_metal_roots_and_their_shares(lib):
    rho = np.float32(0.5)
    m = lobe(lib, rho, 0.6)
    a, b, r = axis_frame(m)
    mu = 0.95                                               # inside the cone: sin(theta) = 0.31 < rho
    w = (mu * a + np.sqrt(1 - mu * mu) * b).astype(np.float32)
    out = np.zeros((1, 3), np.float32)
    lib.nee_lobe_pdf_batch(m, 1, w, out)
    pb, t0, t1 = (float(v) for v in out[0])
    assert t0 > 0 and t1 > 0 and pb > 0
    for t in (t0, t1):   # |t w - m| = 1: rho t is a length of sd = c + rho (a unit vector) in this direction
        assert abs(np.linalg.norm(t * w.astype(np.float64) - m.astype(np.float64)) - 1.0) < 1e-5
    us = (np.arange(20000, dtype=np.uint64) * 214748 + 77).astype(np.uint32)
    lens = np.array([lib.nee_vertex_len_c(float(rho), lib.nee_pick_root_c(t0, t1, int(u)), int(u)) for u in us])
    f0, f1 = np.float32(rho) * np.float32(t0), np.float32(rho) * np.float32(t1)
    assert set(np.unique(lens)) <= {float(f0), float(f1)}
    assert abs(float((lens == float(f0)).mean()) - t0 * t0 / (t0 * t0 + t1 * t1)) < 0.01
    # ... and the shares of the scatter's own lengths in a narrow cone of directions around w agree
    n = 2_000_000
    sc = np.zeros((n, 4), np.float32)
    lib.metal_scatter_dirs(incidence(0.6), NN, rho, 99, n, sc)
    near = sc[:, :3].astype(np.float64) @ w.astype(np.float64) > np.cos(0.02)
    assert near.sum() > 500
    far_root = np.abs(sc[near, 3] - max(f0, f1)) < np.abs(sc[near, 3] - min(f0, f1))
    big, small = max(t0, t1), min(t0, t1)
    assert abs(far_root.mean() - big * big / (big * big + small * small)) < 4.0 * 0.5 / np.sqrt(near.sum()) + 0.02


def test_vertex_pdf_applies_the_acceptance_and_the_codes(lib):
    rho = np.float32(0.8)
    m = lobe(lib, rho, 1.3)                                  # grazing: part of the lobe's cone lies below the surface
    N = np.array([*m, 1.0], np.float32)
    rng = np.random.default_rng(3)
    w = rng.normal(size=(4000, 3)); w /= np.linalg.norm(w, axis=1, keepdims=True)
    w = np.ascontiguousarray(w, np.float32)
    raw = np.zeros((len(w), 3), np.float32); lib.nee_lobe_pdf_batch(m, len(w), w, raw)
    got = np.zeros((len(w), 3), np.float32); lib.nee_vertex_pdf_batch(N, np.array([*NN, rho], np.float32), len(w), w, got)
    up = w[:, 1] > 0
    assert (got[~up, 0] == 0).all() and np.array_equal(got[up], raw[up])
    assert ((raw[:, 0] > 0) & ~up).any() and ((raw[:, 0] > 0) & up).any()
    # code < 0: the isotropic density, one root of length 1 (the length itself is nee_vertex_len's)
    iso = np.zeros((len(w), 3), np.float32); lib.nee_vertex_pdf_batch(N, np.array([0, 0, 0, -1], np.float32), len(w), w, iso)
    assert np.allclose(iso[:, 0], 1.0 / (4.0 * np.pi), rtol=1e-6) and (iso[:, 1] == 1).all() and (iso[:, 2] == 0).all()
    # code 0: the Lambertian density of the normal in N (c / pi for a unit normal)
    lam = np.zeros((len(w), 3), np.float32)
    lib.nee_vertex_pdf_batch(np.array([0, 1, 0, 1], np.float32), np.zeros(4, np.float32), len(w), w, lam)
    assert np.allclose(lam[up, 0], w[up, 1] / np.pi, rtol=1e-4, atol=1e-7) and (lam[~up, 0] == 0).all()
    assert lib.nee_vertex_len_c(0.0, 1.25, 12345) == 1.25


@pytest.mark.parametrize("rho,angle", [(0.5, 1.2), (0.9, 1.35), (1.0, 0.9), (0.3, 1.5), (0.6, 0.2)])
def test_survival_probability_matches_the_scatter(lib, rho, angle):
    # a Metal vertex exists (and samples a light) only when dot(sd, nn) > 0: nee_vertex_inv_acc is 1 / that probability
    m = lobe(lib, np.float32(rho), angle)
    n = 400_000
    out = np.zeros((n, 4), np.float32)
    lib.metal_scatter_dirs(incidence(angle), NN, np.float32(rho), 4242, n, out)
    share = float((out[:, 1] > 0).mean())
    inv = lib.nee_vertex_inv_acc_c(np.array([*m, 1.0], np.float32), np.array([*NN, rho], np.float32))
    expect = min(1.0, 0.5 * (1.0 + float(m[1])))
    assert np.isclose(1.0 / inv, expect, rtol=1e-5)
    assert abs(share - expect) < 5.0 * np.sqrt(max(expect * (1 - expect), 1e-6) / n) + 1e-6, (share, expect)
    # Lambertian and Isotropic vertices always survive
    assert lib.nee_vertex_inv_acc_c(np.array([0, 1, 0, 1], np.float32), np.zeros(4, np.float32)) == 1.0
    assert lib.nee_vertex_inv_acc_c(np.array([0, 0, 0, 1], np.float32), np.array([0, 0, 0, -1], np.float32)) == 1.0


def _cdf_distance(x, cdf):
    x = np.sort(x)
    n = len(x)
    c = cdf(x)
    return max(np.abs(c - np.arange(n) / n).max(), np.abs(c - (np.arange(n) + 1) / n).max())


def test_medium_density_and_length_law(lib):
    n = 400_000
    out = np.zeros((n, 4), np.float32)
    lib.ball_scatter_dirs(777, n, out)
    # direction: uniform on the sphere, 1 / (4 pi) -- each coordinate of a uniform direction is uniform on [-1, 1]
    for k in range(3):
        hist = np.histogram(out[:, k], np.linspace(-1, 1, 41))[0]
        chi2 = ((hist - n / 40.0) ** 2 / (n / 40.0)).sum()
        assert chi2 < 39 + 6.0 * np.sqrt(2.0 * 39), (k, chi2)
    # length: |ballRand| has the CDF r^3; histogram in 40 equal-probability bins, and a Kolmogorov distance
    edges = np.cbrt(np.linspace(0.0, 1.0, 41))
    for name, r in (("ball_rand", out[:, 3].astype(np.float64)),
                    ("nee_vertex_len", np.array([lib.nee_vertex_len_c(-1.0, 1.0, int(u)) for u in
                                                 np.random.default_rng(8).integers(0, 2**32, 100_000, dtype=np.uint64)], np.float64))):
        hist = np.histogram(np.clip(r, 0.0, 1.0), edges)[0]
        e = len(r) / 40.0
        chi2 = ((hist - e) ** 2 / e).sum()
        assert chi2 < 39 + 6.0 * np.sqrt(2.0 * 39), (name, chi2)
        assert _cdf_distance(r, lambda x: x ** 3) < 2.0 / np.sqrt(len(r)), name
    # the helper is cbrt(u01(u)) of the word it is given
    for u in (0x80000000, 0x12345678, 0xFFFFFFFF):
        assert np.isclose(lib.nee_vertex_len_c(-1.0, 1.0, u), np.cbrt((u >> 8) * 2.0 ** -24), rtol=1e-6)


def test_eligibility_at_and_below_rho_min(lib):
    rho_min = lib.nee_rho_min()
    below = float(np.nextafter(np.float32(rho_min), np.float32(0)))
    out = np.zeros(7, np.float32)
    i = incidence(0.4)
    assert lib.scatter_lobe(MAT_METAL, rho_min, i, NN, out) == LOBE_METAL and out[0] == np.float32(rho_min)
    refl = i.astype(np.float64) / np.linalg.norm(i) * [1, -1, 1]
    assert np.allclose(out[1:4], refl + 2.0 ** -23, atol=1e-6) and np.array_equal(out[4:7], NN)
    assert lib.scatter_lobe(MAT_METAL, below, i, NN, out) == LOBE_NONE
    assert lib.scatter_lobe(MAT_METAL, 0.0, i, NN, out) == LOBE_NONE                  # the mirror
    assert lib.scatter_lobe(MAT_METAL, -0.3, i, NN, out) == LOBE_METAL and out[0] == np.float32(0.3)   # |roughness|
    assert lib.scatter_lobe(MAT_METAL, 7.0, i, NN, out) == LOBE_METAL and out[0] == 1.0                 # min(., 1)
    # met from behind its normal (a mesh normal quirk Q-3 left unflipped): m . nn < 0, 1 / P_acc would be unbounded -- not eligible
    assert lib.scatter_lobe(MAT_METAL, 0.5, i * np.array([1, -1, 1], np.float32), NN, out) == LOBE_NONE
    assert lib.scatter_lobe(MAT_ISOTROPIC, 0.0, i, NN, out) == LOBE_MEDIUM
    for kind in (MAT_LAMBERTIAN, MAT_DIELECTRIC, MAT_UVTEST):
        assert lib.scatter_lobe(kind, 0.5 if kind != MAT_DIELECTRIC else 1.5, i, NN, out) == LOBE_NONE


def test_mis_weights_are_unchanged(lib):
    for pb, q in [(1.0, 1.0), (0.3, 2.0), (5.0, 0.01), (1300.0, 0.2), (1e-30, 1e30), (3e38, 3e38), (float("inf"), 1.0)]:
        wb, ws = lib.nee_mis_bsdf_c(pb, q), lib.nee_mis_shadow_c(pb, q)
        assert np.isfinite(wb) and np.isfinite(ws) and 0.0 <= wb <= 1.0 and 0.0 <= ws <= 0.5
        if pb < 1e30 and q < 1e30:
            assert np.isclose(wb, pb * pb / (pb * pb + q * q), rtol=1e-6, atol=1e-30)
            assert np.isclose(ws, pb * q / (pb * pb + q * q), rtol=1e-6, atol=1e-30)
