"""Next-event estimation (HRT_FLAG_NEE) without a GPU: the device functions of hrt_device.h compiled for the host
(tests/tools/nee_on_cpu.cpp) against numpy -- the density p_b of material_scatter's own scatter for normals of any length, the root
choice of the shadow ray, the light samplers and their densities, the MIS weights."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
U = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
I = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
XZ_RECT, XY_RECT, YZ_RECT, SPHERE = 2, 1, 3, 0


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("nee") / "libneecpu.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-shared", "-o", so,
                           os.path.join(HERE, "tools", "nee_on_cpu.cpp")])
    L = C.CDLL(so)
    L.nee_bsdf_pdf_batch.argtypes = [F, C.c_int64, F, F]
    L.scatter_dirs.argtypes = [F, C.c_uint32, C.c_int64, F]
    L.nee_pick_root_c.argtypes = [C.c_float, C.c_float, C.c_uint32]
    L.nee_pick_root_c.restype = C.c_float
    for f in (L.nee_mis_bsdf_c, L.nee_mis_shadow_c):
        f.argtypes = [C.c_float, C.c_float]
        f.restype = C.c_float
    L.nee_sample_batch.argtypes = [F, F, C.c_int64, U, U, I, F]
    L.nee_pdf_batch.argtypes = [F, F, C.c_int64, F, F, F]
    L.nee_choose_c.argtypes = [F, C.c_int, C.c_uint32]
    return L


def normal(r):
    d = np.array([0.3, -0.5, 0.8])
    return (d / np.linalg.norm(d) * r).astype(np.float32)


def pdf(lib, n, w):
    w = np.ascontiguousarray(w, np.float32)
    out = np.zeros((len(w), 3), np.float32)
    lib.nee_bsdf_pdf_batch(n, len(w), w, out)
    return out


def dirs_at(n, mu):
    """unit directions at cosine mu to n's axis (for r = 0 any axis), mu an array"""
    a = normal(1.0).astype(np.float64)
    b = np.cross(a, [1.0, 0.0, 0.0]); b /= np.linalg.norm(b)
    s = np.sqrt(np.maximum(0.0, 1.0 - mu * mu))
    return mu[:, None] * a[None, :] + s[:, None] * b[None, :]


def p_of_mu(lib, n, mu):
    return pdf(lib, n, dirs_at(n, mu))[:, 0].astype(np.float64)


@pytest.mark.parametrize("r", [0.0, 0.3, 1.0, 1.7])
def test_pb_integrates_to_one(lib, r):
    # p_b depends on the angle to n only: integral = 2 pi * int_{-1}^{1} p_b(mu) dmu (midpoint rule; for r > 1 the density has an
    # integrable 1 / sqrt(D) edge at the cone the sphere of sd subtends)
    n = normal(r)
    k = 2_000_000
    mu = -1.0 + (np.arange(k) + 0.5) * (2.0 / k)
    total = 2.0 * np.pi * p_of_mu(lib, n, mu).sum() * (2.0 / k)
    assert abs(total - 1.0) < (2e-3 if r > 1.0 else 2e-4), total


def test_pb_special_values(lib):
    mu = np.array([0.9, 0.5, 0.1, -0.5])
    assert np.allclose(p_of_mu(lib, normal(1.0), mu)[:3], mu[:3] / np.pi, rtol=1e-4)
    assert p_of_mu(lib, normal(1.0), mu)[3] == 0.0                   # below the surface
    assert np.allclose(p_of_mu(lib, normal(0.0), mu), 1.0 / (4.0 * np.pi), rtol=1e-5)


@pytest.mark.parametrize("r", [0.3, 1.0, 1.7])
def test_pb_matches_the_scatter_histogram(lib, r):
    # normalize(n + spherical_rand) drawn with the product's own RNG, binned by mu = w . n / |n|; the expected share of every bin
    # comes from p_b alone.  Chi-square against its degrees of freedom.
    n = normal(r)
    m = 400_000
    w = np.zeros((m, 3), np.float32)
    lib.scatter_dirs(n, 12345, m, w)
    mu = w.astype(np.float64) @ (n.astype(np.float64) / np.linalg.norm(n))
    edges = np.linspace(-1.0, 1.0, 41)
    hist = np.histogram(np.clip(mu, -1.0, 1.0), edges)[0]
    k = 400_000
    grid = -1.0 + (np.arange(k) + 0.5) * (2.0 / k)
    dens = 2.0 * np.pi * p_of_mu(lib, n, grid) * (2.0 / k)
    expect = np.array([dens[(grid >= a) & (grid < b)].sum() for a, b in zip(edges[:-1], edges[1:])]) * m
    keep = expect > 20.0
    assert hist[~keep].sum() <= max(40, 3 * expect[~keep].sum())   # (bins the density leaves empty stay nearly empty)
    chi2 = (((hist[keep] - expect[keep]) ** 2) / expect[keep]).sum()
    dof = keep.sum() - 1
    assert chi2 < dof + 6.0 * np.sqrt(2.0 * dof), (chi2, dof)


def test_roots_and_their_shares(lib):
    n = normal(1.7)
    w = dirs_at(n, np.array([0.95]))
    pb, t0, t1 = pdf(lib, n, w)[0]
    assert t0 > 0 and t1 > 0 and pb > 0
    for t in (t0, t1):   # |t w - n| = 1: both are lengths of sd = n + (a unit vector) in this direction
        assert abs(np.linalg.norm(t * w[0] - n.astype(np.float64)) - 1.0) < 1e-5
    us = (np.arange(20000, dtype=np.uint64) * 214748 + 77).astype(np.uint32)
    picks = np.array([lib.nee_pick_root_c(float(t0), float(t1), int(u)) for u in us])
    share0 = float((picks == t0).mean())
    assert abs(share0 - t0 * t0 / (t0 * t0 + t1 * t1)) < 0.01
    assert set(np.unique(picks)) <= {t0, t1}
    # one positive root (r <= 1): it is always the one
    n1 = normal(0.3)
    _, a, b = pdf(lib, n1, w)[0]
    assert a > 0 and b == 0
    assert lib.nee_pick_root_c(float(a), float(b), 0xFFFFFFFF) == a


def light(kind, p, area):
    rec = np.zeros(12, np.float32)
    rec[[0, 1]] = np.array([7, kind], np.int32).view(np.float32)
    rec[2], rec[3] = 1.0, 1.0
    rec[4:8] = p[:4]
    rec[8] = p[4] if kind != SPHERE else 0.0
    rec[9] = area
    return rec


def sample(lib, L, x, m=4000):
    rng = np.random.default_rng(5)
    uy = rng.integers(0, 2**32, m, dtype=np.uint64).astype(np.uint32)
    uz = rng.integers(0, 2**32, m, dtype=np.uint64).astype(np.uint32)
    ok = np.zeros(m, np.int32)
    out = np.zeros((m, 5), np.float32)
    lib.nee_sample_batch(L, x, m, uy, uz, ok, out)
    return ok.astype(bool), out


def check_pdf(lib, L, x, w, pl, y):
    got = np.zeros(len(w), np.float32)
    lib.nee_pdf_batch(L, x, len(w), np.ascontiguousarray(w, np.float32), np.ascontiguousarray(y, np.float32), got)
    assert np.allclose(got, pl, rtol=2e-4), np.abs(got / pl - 1).max()


@pytest.mark.parametrize("kind,axis", [(XZ_RECT, 1), (XY_RECT, 2), (YZ_RECT, 0)])
def test_rect_samples_lie_on_the_light(lib, kind, axis):
    p = np.array([-1.0, 2.0, 0.5, 1.5, 3.0], np.float32)            # a0, a1, b0, b1, k
    L = light(kind, p, 3.0)
    for x in (np.array([0.2, -0.4, 0.1], np.float32), np.array([0.3, 5.0, 4.0], np.float32)):
        ok, out = sample(lib, L, x)
        assert ok.all()
        w, pl, reach = out[:, :3].astype(np.float64), out[:, 3], out[:, 4].astype(np.float64)
        # the point on the rect's plane along w (float64), inside the rect
        s = (3.0 - x[axis]) / w[:, axis]
        y = x[None, :] + s[:, None] * w
        others = [k for k in range(3) if k != axis]
        a, b = y[:, others[0]], y[:, others[1]]
        assert (a >= -1.0 - 1e-4).all() and (a <= 2.0 + 1e-4).all() and (b >= 0.5 - 1e-4).all() and (b <= 1.5 + 1e-4).all()
        assert np.allclose(s, reach, rtol=1e-5)
        # pl = dist^2 / (A |cos|), and the same from the direction alone
        assert np.allclose(pl, s * s / (3.0 * np.abs(w[:, axis])), rtol=1e-4)
        check_pdf(lib, L, x, w, pl, y)
        # uniform over the rect: the sampled points' mean is the centre
        assert abs(a.mean() - 0.5) < 0.05 and abs(b.mean() - 1.0) < 0.02


def sphere_hits(x, w, c, r):
    oc = x[None, :] - c[None, :]
    b = (oc * w).sum(1)
    disc = b * b - ((oc * oc).sum(1) - r * r)
    return b, disc


def test_sphere_samples_from_outside(lib):
    c, r = np.array([1.0, 2.0, -1.0]), 0.75
    L = light(SPHERE, np.array([*c, r, 0.0], np.float32), 4 * np.pi * r * r)
    x = np.array([3.0, -1.0, 0.5], np.float32)
    ok, out = sample(lib, L, x)
    assert ok.all()
    w, pl = out[:, :3].astype(np.float64), out[:, 3]
    b, disc = sphere_hits(x.astype(np.float64), w, c, r)
    assert (disc > -1e-5 * r * r).all()                            # every direction meets the sphere
    dc2 = ((c - x) ** 2).sum()
    omc = 1.0 - np.sqrt(1.0 - r * r / dc2)
    assert np.allclose(pl, 1.0 / (2.0 * np.pi * omc), rtol=1e-4)
    # uniform in the cone: cos theta to the axis is uniform in [cos theta_max, 1]
    a = (c - x) / np.sqrt(dc2)
    ct = w @ a
    assert abs(ct.mean() - (1.0 - omc / 2.0)) < 0.02 * omc
    y = x[None, :] + (-b - np.sqrt(np.maximum(disc, 0.0)))[:, None] * w
    check_pdf(lib, L, x, w, pl, y)


def test_sphere_samples_from_inside(lib):
    c, r = np.array([0.0, 1.0, 0.0]), 2.0
    L = light(SPHERE, np.array([*c, r, 0.0], np.float32), 4 * np.pi * r * r)
    x = np.array([0.5, 0.7, -0.3], np.float32)
    ok, out = sample(lib, L, x)
    assert ok.all()
    w, pl, reach = out[:, :3].astype(np.float64), out[:, 3], out[:, 4].astype(np.float64)
    y = x[None, :] + reach[:, None] * w
    assert np.allclose(np.linalg.norm(y - c[None, :], axis=1), r, rtol=1e-5)   # on the surface
    cl = np.abs(((y - c[None, :]) * w).sum(1)) / r
    assert np.allclose(pl, reach * reach / (4 * np.pi * r * r * cl), rtol=1e-4)
    check_pdf(lib, L, x, w, pl, y)


def test_mis_weights(lib):
    for pb, q in [(1.0, 1.0), (0.3, 2.0), (5.0, 0.01), (1e-30, 1e30), (3e38, 3e38), (float("inf"), 1.0), (1.0, float("inf"))]:
        wb, ws = lib.nee_mis_bsdf_c(pb, q), lib.nee_mis_shadow_c(pb, q)
        assert np.isfinite(wb) and np.isfinite(ws) and 0.0 <= wb <= 1.0 and 0.0 <= ws <= 0.5
        if pb < 1e30 and q < 1e30:
            assert np.isclose(wb, pb * pb / (pb * pb + q * q), rtol=1e-6, atol=1e-30)
            assert np.isclose(ws, pb * q / (pb * pb + q * q), rtol=1e-6, atol=1e-30)
    assert lib.nee_mis_bsdf_c(0.0, 1.0) == 0.0 and lib.nee_mis_bsdf_c(1.0, 0.0) == 1.0
    assert lib.nee_mis_shadow_c(0.0, 1.0) == 0.0 and lib.nee_mis_shadow_c(1.0, 0.0) == 0.0


def test_light_choice_follows_the_cdf(lib):
    table = np.zeros(3 * 12, np.float32)
    table[3::12][:3] = [0.25, 0.375, 1.0]
    us = (np.arange(4096, dtype=np.uint64) << np.uint64(20)).astype(np.uint32)
    picks = np.array([lib.nee_choose_c(table, 3, int(u)) for u in us])
    assert np.allclose(np.bincount(picks, minlength=3) / len(us), [0.25, 0.125, 0.625], atol=1e-3)
