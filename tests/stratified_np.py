"""numpy restatement (uint32 arithmetic) of HRT_FLAG_STRATIFIED's sampler, written from the comment block of csrc/hrt_rng.h and
DESIGN.md 4.9 alone, on top of tests/f64_reference.py's Philox: nothing here is shared with the header, so a misreading of the layout
cannot hide in both.  sobol2 is the plain 32-XOR loop over the direction numbers, not the header's masked shifts."""
import numpy as np

from tests import f64_reference as F

RNG_LIGHT, RNG_ENV = 6, 7
SEEDS_SAMPLE, SEEDS_BIT = 0xFFFFFFFF, 0x80000000
_U = np.uint32


def brev(v):
    v = np.asarray(v, np.uint32).copy()
    v = (v >> _U(16)) | (v << _U(16))
    v = ((v & _U(0xFF00FF00)) >> _U(8)) | ((v & _U(0x00FF00FF)) << _U(8))
    v = ((v & _U(0xF0F0F0F0)) >> _U(4)) | ((v & _U(0x0F0F0F0F)) << _U(4))
    v = ((v & _U(0xCCCCCCCC)) >> _U(2)) | ((v & _U(0x33333333)) << _U(2))
    return ((v & _U(0xAAAAAAAA)) >> _U(1)) | ((v & _U(0x55555555)) << _U(1))


def lk(x, seed):
    """Laine-Karras permutation with Burley's constants, mod 2^32"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, np.uint32) + np.asarray(seed, np.uint32)
        for c in (0x6c50b47c, 0xb82f1e52, 0xc7afe638, 0x8d22f6e6):
            x = x ^ (x * _U(c))
    return x


def nus(x, seed):
    return brev(lk(brev(x), seed))


def sobol2(j):
    """Sobol's second dimension: v_0 = 1 << 31, v_k = v_{k-1} ^ (v_{k-1} >> 1); the XOR of v_k over the set bits k of j"""
    j = np.asarray(j, np.uint32)
    out = np.zeros_like(j)
    v = _U(1 << 31)
    for k in range(32):
        out ^= np.where((j >> _U(k)) & _U(1), v, _U(0)).astype(np.uint32)
        v = v ^ (v >> _U(1))
    return out


def mix(x):
    with np.errstate(over="ignore"):
        x = np.asarray(x, np.uint32).copy()
        x ^= x >> _U(16); x = x * _U(0x7feb352d)
        x ^= x >> _U(15); x = x * _U(0x846ca68b)
        x ^= x >> _U(16)
    return x


def net(sample, sa, sb, sc):
    j = nus(np.asarray(sample, np.uint32), sa)
    return nus(brev(j), sb), nus(sobol2(j), sc)


def seeds(seed_lo, seed_hi, pixel, bounce, purpose, aux=0):
    word3 = np.uint64(purpose) | (np.asarray(aux, dtype=np.uint64) << np.uint64(8)) | np.uint64(SEEDS_BIT)
    return F.philox4x32_10(pixel, SEEDS_SAMPLE, bounce, word3, seed_lo, seed_hi)


def draw(seed_lo, seed_hi, pixel, sample, bounce, purpose, aux=0):
    """the stratified twin of f64_reference.draw: 4 uint32 arrays x, y, z, w (every argument broadcasts)"""
    k = seeds(seed_lo, seed_hi, pixel, bounce, purpose, aux)
    sample = np.broadcast_to(np.asarray(sample, np.uint32), np.broadcast(np.asarray(pixel), np.asarray(sample), np.asarray(bounce)).shape)
    a0, a1 = net(sample, k[0], k[1], k[2])
    with np.errstate(over="ignore"):
        b0, b1 = net(sample, mix(k[3] + _U(0x9E3779B9)), mix(k[3] + _U(0x3C6EF372)), mix(k[3] + _U(0xDAA66D2B)))
    if purpose == RNG_LIGHT and np.all(np.asarray(aux) == 0):
        return b0, a0, a1, b1
    return a0, a1, b0, b1
