"""Environment-map importance sampling (HRT_FLAG_NEE_ENV) without a GPU: the device functions of hrt_device.h env_*
compiled for the host (tests/tools/env_on_cpu.cpp) against numpy float64 tables (tests/env_tables.py) -- the cells of the reference's
nearest-texel lookup and their solid angles, the texel weights, the sampler (it draws cells with the table's probabilities and never a
dark one) and the density, the MIS weights for a very bright texel, and maps without a table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import env_tables as et

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
D = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
I = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("env") / "libenvcpu.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-shared", "-o", so,
                           os.path.join(HERE, "tools", "env_on_cpu.cpp")])
    L = C.CDLL(so)
    L.env_cells.argtypes = [C.c_int, C.c_int, C.c_void_p, F]
    L.env_cell_of_batch.argtypes = [C.c_int, C.c_int, C.c_int64, F, I]
    L.env_sample_batch.argtypes = [F, F, C.c_int, C.c_int, C.c_uint32, C.c_int64, I, I, F, F]
    L.env_pdf_batch.argtypes = [F, F, C.c_int, C.c_int, C.c_int64, F, F]
    L.env_weights.argtypes = [F, C.c_int, C.c_int, C.c_int, D]
    for f in (L.env_mis_bsdf_c, L.env_mis_shadow_c):
        f.argtypes = [C.c_float, C.c_float]
        f.restype = C.c_float
    return L


def omega(lib, W, H):
    out = np.zeros(W * H, np.float32)
    lib.env_cells(W, H, None, out)
    return out.reshape(H, W)


def pdf(lib, marg, cond, d):
    d = np.ascontiguousarray(d.reshape(-1, 3), np.float32)
    out = np.zeros(len(d), np.float32)
    lib.env_pdf_batch(marg, np.ascontiguousarray(cond), cond.shape[1] - 1, len(marg) - 1, len(d), d, out)
    return out


def sample(lib, marg, cond, n, seed):
    ok = np.zeros(n, np.int32)
    ij = np.zeros((n, 2), np.int32)
    w = np.zeros((n, 3), np.float32)
    p = np.zeros(n, np.float32)
    lib.env_sample_batch(marg, np.ascontiguousarray(cond), cond.shape[1] - 1, len(marg) - 1, seed, n, ok, ij, w, p)
    return ok, ij, w, p


def cell_of(lib, W, H, d):
    d = np.ascontiguousarray(d.reshape(-1, 3), np.float32)
    ij = np.zeros((len(d), 2), np.int32)
    lib.env_cell_of_batch(W, H, len(d), d, ij)
    return ij


@pytest.mark.parametrize("W,H", [(1, 1), (2, 2), (7, 5), (64, 32), (4096, 2048)])
def test_cells_cover_the_sphere(lib, W, H):
    om = omega(lib, W, H)
    assert (om > 0).all()
    assert abs(om.astype(np.float64).sum() / (4 * np.pi) - 1.0) < 1e-6
    assert np.allclose(om, et.solid_angles(W, H), rtol=2e-5, atol=0)


@pytest.mark.parametrize("W,H", [(7, 5), (64, 32)])
def test_cell_centres_map_back_to_their_cells(lib, W, H):
    ij = cell_of(lib, W, H, et.centre_directions(W, H)).reshape(H, W, 2)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inner = np.ones((H, W), bool)
    inner[0] = inner[-1] = False         # the poles: every phi is the same direction
    assert (ij[..., 0][inner] == ii[inner]).all() and (ij[..., 1] == jj).all()


def test_weights_match_float64(lib):
    tex = et.messy_map(np.random.default_rng(3), 37, 19)
    out = np.zeros(37 * 19)
    lib.env_weights(np.ascontiguousarray(tex), 37, 19, 3, out)
    ref = et.weights(tex).reshape(-1)
    assert np.allclose(out, ref, rtol=1e-13, atol=0)
    assert (out[ref == 0] == 0).all()


def test_density_integrates_to_one(lib):
    tex = et.messy_map(np.random.default_rng(5), 64, 32)
    marg, cond = et.table(tex)
    p = pdf(lib, marg, cond, et.centre_directions(64, 32)).reshape(32, 64).astype(np.float64)
    total = (p * omega(lib, 64, 32)).sum()
    assert abs(total - 1.0) < 1e-5, total
    assert np.allclose(p * omega(lib, 64, 32), et.cell_probs(marg, cond), rtol=1e-5, atol=1e-12)


def test_dark_texels_have_zero_density(lib):
    tex = et.messy_map(np.random.default_rng(7), 64, 32)
    marg, cond = et.table(tex)
    p = pdf(lib, marg, cond, et.centre_directions(64, 32)).reshape(32, 64)
    dark = et.weights(tex) == 0
    assert dark.sum() > 64 + 32
    assert (p[dark] == 0).all() and (p[~dark] > 0).all()


def test_samples_map_back_to_their_cells(lib):
    tex = et.messy_map(np.random.default_rng(11), 64, 32)
    marg, cond = et.table(tex)
    n = 200_000
    ok, ij, w, p = sample(lib, marg, cond, n, 1)
    assert ok.all()
    assert np.allclose(np.linalg.norm(w, axis=1), 1.0, atol=1e-5)
    back = cell_of(lib, 64, 32, w)
    miss = np.any(back != ij, axis=1)
    assert miss.mean() < 1e-4, miss.sum()
    # the sampler's density is the table's: P(cell) / solid angle
    om = omega(lib, 64, 32)
    assert np.allclose(p, et.cell_probs(marg, cond)[ij[:, 1], ij[:, 0]] / om[ij[:, 1], ij[:, 0]], rtol=1e-5)
    # ... and the density of the direction agrees wherever the lookup lands in the sampled cell
    q = pdf(lib, marg, cond, w)
    assert np.allclose(q[~miss], p[~miss], rtol=1e-5)


def test_sampled_cells_follow_the_table(lib):
    tex = et.messy_map(np.random.default_rng(13), 24, 12)
    marg, cond = et.table(tex)
    P = et.cell_probs(marg, cond).astype(np.float64)
    n = 400_000
    ok, ij, _, _ = sample(lib, marg, cond, n, 2)
    assert ok.all()
    counts = np.zeros_like(P)
    np.add.at(counts, (ij[:, 1], ij[:, 0]), 1)
    assert counts[P == 0].sum() == 0                  # no cell of weight 0 is ever drawn
    assert counts[et.weights(tex) == 0].sum() == 0
    e = n * P
    m = e >= 5
    chi2 = ((counts[m] - e[m]) ** 2 / e[m]).sum()
    dof = m.sum() - 1
    assert (chi2 - dof) / np.sqrt(2 * dof) < 5.0, (chi2, dof)


def test_mis_weights_stay_finite_for_a_sun(lib):
    for W, H, j in ((4096, 2048, 700), (512, 256, 0), (64, 32, 31)):
        tex = np.zeros((H, W, 3), np.float32)
        tex[j, W // 3] = 1e6
        marg, cond = et.table(tex)
        d = et.centre_directions(W, H)[j, W // 3]
        q = float(pdf(lib, marg, cond, d)[0])
        assert q > 0 and np.isfinite(q)
        assert abs(q * omega(lib, W, H)[j, W // 3] - 1.0) < 1e-5
        for pb in (0.0, 1e-7, 1e-3, 1 / np.pi, 0.9, 1e3):
            b, s = lib.env_mis_bsdf_c(pb, q), lib.env_mis_shadow_c(pb, q)
            assert np.isfinite(b) and np.isfinite(s) and 0.0 <= b <= 1.0 and 0.0 <= s <= 0.5, (pb, q, b, s)
            assert abs(b + s * q / pb - 1.0) < 1e-5 if pb > 0 else b == 0.0


@pytest.mark.parametrize("kind", ["zero", "nan", "negative"])
def test_maps_without_a_table(lib, kind):
    W, H = 16, 8
    tex = np.full((H, W, 3), {"zero": 0.0, "nan": np.nan, "negative": -2.0}[kind], np.float32)
    out = np.zeros(W * H)
    lib.env_weights(tex, W, H, 3, out)
    assert (out == 0).all()
    assert et.table(tex) is None
