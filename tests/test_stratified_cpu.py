"""HRT_FLAG_STRATIFIED's sampler without a GPU: the functions of csrc/hrt_rng.h compiled for the host
(tests/tools/sampler_on_cpu.cpp).  The net property is exact -- Owen scrambling keeps every elementary interval of a (0,2)-sequence's
aligned blocks at exactly one point -- so those tests have no tolerance; marginals and independence across draw sites are chi-square
tests with the threshold tests/test_nee_cpu.py uses; the default sampler is compared bit for bit with tests/f64_reference.py's Philox."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import f64_reference as F
from tests import stratified_np as SN

HERE = os.path.dirname(os.path.abspath(__file__))
U = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
RNG_JITTER, RNG_SCATTER, RNG_LENS, RNG_LIGHT, RNG_ENV = 0, 1, 5, 6, 7
PHILOX, STRAT, SEEDS = 0, 1, 2

# (purpose, aux, bounces, the word pairs that choose ONE 2-D quantity, further pairs that are one net as well)
SITES = [
    (RNG_JITTER, 0, (0,), [(0, 1)], []),                 # the point in the pixel
    (RNG_SCATTER, 0, (0, 1, 7), [(0, 1)], [(2, 3)]),     # sphericalRand; the Fresnel coin's two words
    (RNG_LIGHT, 0, (0, 2, 5), [(1, 2)], [(0, 3)]),       # the point on the light; light choice and root choice
    (RNG_ENV, 0, (0, 3), [(0, 1), (2, 3)], []),          # row / column; the position in the cell
    (RNG_LENS, 0, (0,), [], []),                         # 1-D: the angle on the lens
    (RNG_LIGHT, 1, (1,), [], []),                        # 1-D: the alias coin
    (RNG_ENV, 1, (4,), [], []),                          # 1-D: the root choice
]
SEEDS_PIXELS = [(0x1, 0x0, 0), (0x9ABCDEF0, 0x12345678, 640 * 231 + 17), (0xFFFFFFFF, 0xFFFFFFFF, 1920 * 1080 - 1), (0xC0FFEE, 0x7, 4097)]
K_MAX = 10
BLOCKS = (0, 1, 6, 85, (1 << 16) + 3)        # block numbers: block b of size 2^k holds the samples [b 2^k, (b + 1) 2^k); the last lies beyond 2^16


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sampler") / "libsamplercpu.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-shared", "-o", so,
                           os.path.join(HERE, "tools", "sampler_on_cpu.cpp")])
    L = C.CDLL(so)
    L.sampler_draw.argtypes = [C.c_uint32, C.c_uint32, C.c_int64, U, U, C.c_int]
    for f in (L.strat_brev_c, L.strat_pascal_c, L.strat_mix_c):
        f.argtypes = [C.c_uint32]; f.restype = C.c_uint32
    L.strat_lk_c.argtypes = [C.c_uint32, C.c_uint32]; L.strat_lk_c.restype = C.c_uint32
    return L


def draws(lib, seed_lo, seed_hi, pixel, sample, bounce, purpose, aux=0, which=STRAT):
    """-> uint32 [n, 4]; pixel / sample / bounce broadcast"""
    pixel, sample, bounce = np.broadcast_arrays(np.asarray(pixel, np.uint32), np.asarray(sample, np.uint32), np.asarray(bounce, np.uint32))
    keys = np.empty((pixel.size, 4), np.uint32)
    keys[:, 0] = pixel.ravel(); keys[:, 1] = sample.ravel(); keys[:, 2] = bounce.ravel(); keys[:, 3] = purpose | (aux << 8)
    out = np.zeros_like(keys)
    lib.sampler_draw(seed_lo, seed_hi, len(keys), keys, out, which)
    return out


def all_sites():
    for seed_lo, seed_hi, pixel in SEEDS_PIXELS:
        for purpose, aux, bounces, pairs, more in SITES:
            for b in bounces:
                yield seed_lo, seed_hi, pixel, b, purpose, aux, pairs + more


def test_there_are_enough_sites():
    sites = list(all_sites())
    assert len(sites) >= 32 and sum(1 for s in sites if s[6]) >= 32


def test_every_aligned_block_is_a_net_and_every_word_a_stratified_sequence(lib):
    """k = 0..10, every aligned block [b 2^k, (b + 1) 2^k) of sample indexes for the block numbers BLOCKS, every split 2^a x 2^(k - a): each
    elementary interval holds exactly one point, on the 24-bit values u01 sees; and each word alone hits each of the 2^k intervals once."""
    checks = 0
    for seed_lo, seed_hi, pixel, bounce, purpose, aux, pairs in all_sites():
        for k in range(K_MAX + 1):
            n = 1 << k
            for b in BLOCKS:
                s = (np.uint32(b) << np.uint32(k)) + np.arange(n, dtype=np.uint32)
                v = draws(lib, seed_lo, seed_hi, pixel, s, bounce, purpose, aux) >> np.uint32(8)          # 24-bit values
                for word in range(4):
                    cells = v[:, word] >> np.uint32(24 - k)
                    assert len(np.unique(cells)) == n, (seed_lo, pixel, bounce, purpose, aux, "word", word, k, b)
                    checks += 1
                for (p, q) in pairs:
                    for a in range(k + 1):
                        cells = ((v[:, p] >> np.uint32(24 - a)).astype(np.uint64) << np.uint64(k - a)) | (v[:, q] >> np.uint32(24 - (k - a)))
                        assert len(np.unique(cells)) == n, (seed_lo, pixel, bounce, purpose, aux, (p, q), k, a, b)
                        checks += 1
    print(f"{checks} exact checks")


def _chi2_ok(counts, expected):
    dof = counts.size - 1
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    return chi2 < dof + 6.0 * np.sqrt(2.0 * dof), chi2


@pytest.mark.parametrize("purpose,aux", [(RNG_JITTER, 0), (RNG_SCATTER, 0), (RNG_LENS, 0), (RNG_LIGHT, 0), (RNG_LIGHT, 1), (RNG_ENV, 0), (RNG_ENV, 1)])
@pytest.mark.parametrize("sample", [0, 5, 70001])
def test_marginals_are_uniform_over_pixels(lib, purpose, aux, sample):
    n = 1 << 17
    u = draws(lib, 0x51ED, 0x2, np.arange(n), sample, 1, purpose, aux)
    for word in range(4):
        counts = np.bincount(u[:, word] >> np.uint32(26), minlength=64).astype(np.float64)
        ok, chi2 = _chi2_ok(counts, n / 64.0)
        assert ok, (purpose, aux, word, chi2)


def _joint_ok(a, b):
    counts = np.bincount(((a >> np.uint32(29)) << np.uint32(3)) | (b >> np.uint32(29)), minlength=64).astype(np.float64)
    return _chi2_ok(counts, a.size / 64.0)


def test_draw_sites_are_independent_of_each_other(lib):
    n = 1 << 17
    pix = np.arange(n)
    for sample in (0, 9):
        b0 = draws(lib, 0xBEEF, 0x0, pix, sample, 0, RNG_SCATTER)
        b1 = draws(lib, 0xBEEF, 0x0, pix, sample, 1, RNG_SCATTER)
        li = draws(lib, 0xBEEF, 0x0, pix, sample, 0, RNG_LIGHT)
        en = draws(lib, 0xBEEF, 0x0, pix, sample, 0, RNG_ENV)
        ji = draws(lib, 0xBEEF, 0x0, pix, sample, 0, RNG_JITTER)
        for wa in range(4):
            for wb in range(4):
                for name, x, y in (("bounce 0 / 1", b0, b1), ("scatter / light", b0, li), ("scatter / env", b0, en), ("jitter / scatter", ji, b0),
                                   ("light / env", li, en)):
                    ok, chi2 = _joint_ok(x[:, wa], y[:, wb])
                    assert ok, (name, sample, wa, wb, chi2)
        # two samples of one site are NOT independent (that is the point), but the two nets of one draw are
        for wa, wb in ((0, 2), (0, 3), (1, 2), (1, 3)):
            ok, chi2 = _joint_ok(b0[:, wa], b0[:, wb])
            assert ok, ("net A / net B", sample, wa, wb, chi2)


def test_seeds_do_not_depend_on_the_sample(lib):
    pix = np.arange(4096)
    for purpose, aux in ((RNG_JITTER, 0), (RNG_LIGHT, 1), (RNG_ENV, 0)):
        k0 = draws(lib, 0xABCD, 0x1, pix, 0, 2, purpose, aux, SEEDS)
        for sample in (1, 77, 1 << 20):
            assert np.array_equal(k0, draws(lib, 0xABCD, 0x1, pix, sample, 2, purpose, aux, SEEDS))
        # ... and they differ between sites
        assert not np.array_equal(k0, draws(lib, 0xABCD, 0x1, pix, 0, 3, purpose, aux, SEEDS))
        assert not np.array_equal(k0, draws(lib, 0xABCD, 0x1, pix + 1, 0, 2, purpose, aux, SEEDS))
        # the call is one no default draw makes: its counter is the one the header documents
        want = F.philox4x32_10(pix, 0xFFFFFFFF, 2, purpose | (aux << 8) | 0x80000000, 0xABCD, 0x1)
        assert np.array_equal(k0, np.stack(want, axis=-1))


def test_the_default_sampler_is_bit_identical(lib):
    rng = np.random.default_rng(11)
    n = 20000
    pix, smp, bnc = (rng.integers(0, 1 << 32, n, dtype=np.uint64) for _ in range(3))
    bnc[::2] &= np.uint64(63)
    for purpose, aux in ((0, 0), (1, 0), (2, 12345), (3, 7), (5, 0), (6, 0), (6, 1), (7, 0), (7, 1)):
        got = draws(lib, 0x89ABCDEF, 0x01234567, pix, smp, bnc, purpose, aux, PHILOX)
        want = F.draw(0x89ABCDEF, 0x01234567, pix, smp, bnc, purpose, aux)
        assert np.array_equal(got, np.stack(want, axis=-1)), (purpose, aux)


def test_the_numpy_restatement_is_the_header(lib):
    """tests/stratified_np.py (what the float64 pin on the GPU is restated from) against the compiled header, part by part and whole"""
    rng = np.random.default_rng(5)
    v = rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32)
    sd = rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(SN.brev(v), [lib.strat_brev_c(int(x)) for x in v])
    assert np.array_equal(SN.lk(v, sd), [lib.strat_lk_c(int(x), int(s)) for x, s in zip(v, sd)])
    assert np.array_equal(SN.mix(v), [lib.strat_mix_c(int(x)) for x in v])
    # the masked shifts are Sobol's second dimension, bit-reversed
    assert np.array_equal(SN.brev(SN.sobol2(v)), [lib.strat_pascal_c(int(x)) for x in v])
    small = np.arange(4096, dtype=np.uint32)
    assert np.array_equal(SN.brev(SN.sobol2(small)), [lib.strat_pascal_c(int(x)) for x in small])
    n = 5000
    pix, smp = rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 32, n, dtype=np.uint64)
    smp[::3] &= np.uint64(1023)
    bnc = rng.integers(0, 50, n, dtype=np.uint64)
    for purpose, aux in ((RNG_JITTER, 0), (RNG_SCATTER, 0), (RNG_LENS, 0), (RNG_LIGHT, 0), (RNG_LIGHT, 1), (RNG_ENV, 0), (RNG_ENV, 1)):
        got = draws(lib, 0x77, 0x88, pix, smp, bnc, purpose, aux)
        want = SN.draw(0x77, 0x88, pix, smp, bnc, purpose, aux)
        assert np.array_equal(got, np.stack(want, axis=-1)), (purpose, aux)
