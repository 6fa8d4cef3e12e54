"""Host-side helpers of the sparse adaptive-pass tests (tests/test_gpu_adaptive_sparse.py): no GPU in them.

With threshold 0 a pixel is active in pass k >= 1 exactly when count[q] == done (done = min_samples + (k - 1) * pass_samples), so a
test chooses the active set S itself: crafted() puts `done` and the uniform render's running sums into the pixels of S and sentinels
(NaN among them, counts that never equal `done`) into all others; expect() states what the pass must hand back -- the running sums
after done + n samples in S, the input's bits everywhere else; patterns() names the active sets around the sizes at which the
compaction (blocks of AD_ITEMS pixels, scanned in chunks of SCAN_CHUNK block counts) and the list's slot arithmetic change path."""
import numpy as np

AD_ITEMS = 1024          # pixels per block of k_ad_select
SCAN_CHUNK = 256         # block counts per chunk of k_ad_scan
LIST_SIZES = (1, 2, 63, 64, 65, 255, 257, 1025)      # n_list around fastdiv's d == 1, the wave, the block of 256 threads and AD_ITEMS
INT32_MAX = 2**31 - 1


def luma(rgb):
    """Y of hrt.h in float32: three products, added left to right (the library builds with -ffp-contract=off)."""
    rgb = np.asarray(rgb, np.float32)
    return np.float32(0.2126) * rgb[..., 0] + np.float32(0.7152) * rgb[..., 1] + np.float32(0.0722) * rgb[..., 2]


def sum_prefix(rad):
    """rad [spp, ..., 3] per-sample radiance -> [spp + 1, ..., 3]: the float32 running sums, in sample order, from +0."""
    rad = np.asarray(rad, np.float32)
    out = np.zeros((rad.shape[0] + 1,) + rad.shape[1:], np.float32)
    for s in range(rad.shape[0]):
        out[s + 1] = out[s] + rad[s]
    return out


def y2_prefix(rad):
    """rad [spp, ..., 3] per-sample radiance -> [spp + 1, ...]: the float32 running sum, in sample order, of each sample's Y * Y."""
    y = luma(rad)
    yy = y * y
    out = np.zeros((yy.shape[0] + 1,) + yy.shape[1:], np.float32)
    for s in range(yy.shape[0]):
        out[s + 1] = out[s] + yy[s]
    return out


def other_counts(done):
    """Counts a pixel outside the active set may hold: none of them is `done` (done >= 2)."""
    return np.array([0, done - 1, done + 1, -7, INT32_MAX], np.int64).astype(np.int32)


def as_mask(S, shape):
    """S: a boolean mask of `shape` (or of its flattening) or an array of flat pixel indices -> boolean mask of `shape`."""
    S = np.asarray(S)
    if S.dtype == np.bool_:
        return S.reshape(shape).copy()
    m = np.zeros(int(np.prod(shape)), np.bool_)
    m[S.astype(np.int64)] = True
    return m.reshape(shape)


def crafted(prefix_done, sq_done, S_mask, done, seed):
    """-> (sums, sq, count), the buffers that make exactly S active in the pass whose pixels have `done` samples (threshold 0).
    In S: the running sums prefix_done [rows, W, 3] and sq_done [rows, W] and count == done.  Outside S: seeded sentinels -- finite
    numbers, infinities and NaNs in sums and sq (at least one NaN in each whenever a pixel outside S exists) and counts drawn from
    other_counts(done), every one of them present when five pixels outside S exist."""
    assert done >= 2
    shape = sq_done.shape
    S = as_mask(S_mask, shape)
    rng = np.random.default_rng(seed)
    sums = (rng.standard_normal(shape + (3,)) * 100.0).astype(np.float32)
    sq = (rng.standard_normal(shape) * 100.0).astype(np.float32)         # (a negative sq: nothing the device could have written)
    count = rng.choice(other_counts(done), size=shape).astype(np.int32)
    out = np.flatnonzero(~S.ravel())
    if out.size:
        special = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)
        pick = rng.random(out.size) < 0.125
        pick[0] = True
        which = rng.integers(0, special.size, out.size)
        which[0] = 0                                                     # the first pixel outside S: NaN in all of sums and in sq
        fs, fq = sums.reshape(-1, 3), sq.reshape(-1)
        fs[out[pick], rng.integers(0, 3, int(pick.sum()))] = special[which[pick]]
        fs[out[0]] = np.nan
        fq[out[pick]] = special[which[::-1][pick]]
        fq[out[0]] = np.nan
        k = min(out.size, 5)
        count.reshape(-1)[out[:k]] = other_counts(done)[:k]
    sums[S] = prefix_done[S]
    sq[S] = sq_done[S]
    count[S] = done
    return sums, sq, count


def expect(inputs, prefix_after, sq_after, S_mask, done, n):
    """-> (sums, sq, count) the pass must return for the `inputs` of crafted(): in S the running sums after done + n samples and
    count == done + n, everywhere else the inputs' bits."""
    sums, sq, count = (a.copy() for a in inputs)
    S = as_mask(S_mask, sq.shape)
    sums[S] = prefix_after[S]
    sq[S] = sq_after[S]
    count[S] = done + n
    return sums, sq, count


def same_bits(a, b):
    """bit equality of two float32 or int32 arrays (NaNs and signed zeros included)"""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _random_size(n_local, density):
    return int(round(density * n_local))


def pattern_sizes(n_local):
    """name -> the size the name promises, for every pattern patterns(n_local, .) returns: stated from n_local alone."""
    n = int(n_local)
    nb = (n + AD_ITEMS - 1) // AD_ITEMS
    sizes = {"empty": 0}
    if n < 1:
        return sizes
    sizes.update({"first_pixel": 1, "last_pixel": 1, "all": n})
    if n >= 2:
        sizes["first_and_last"] = 2
    for m in LIST_SIZES:
        if m <= n:
            sizes[f"first_{m}"] = m
            sizes[f"last_{m}"] = m
    if n >= AD_ITEMS:
        sizes["mod1024_is_0"] = (n + AD_ITEMS - 1) // AD_ITEMS
        sizes["mod1024_is_1023"] = n // AD_ITEMS
    if n >= 64:
        sizes["mod64_is_63"] = n // 64
    if nb >= 2:
        sizes["all_but_block_0"] = n - AD_ITEMS
        sizes["one_per_block"] = nb
    if nb > SCAN_CHUNK + 1:           # blocks 255 and 256 are whole, and blocks past 256 exist
        sizes["block_255"] = AD_ITEMS
        sizes["block_256"] = AD_ITEMS
        sizes["blocks_255_and_256"] = 2 * AD_ITEMS
        sizes["blocks_from_256"] = n - SCAN_CHUNK * AD_ITEMS
    for name, d in (("random_half", 0.5), ("random_hundredth", 0.01)):
        if _random_size(n, d) >= 1:
            sizes[name] = _random_size(n, d)
    sizes["random_three"] = min(3, n)
    return sizes


def patterns(n_local, seed):
    """name -> sorted flat pixel indices (int64) of the active sets the sparse tests render on a film of n_local local pixels; a
    set the film is too small for is left out ("empty" is always there)."""
    n = int(n_local)
    nb = (n + AD_ITEMS - 1) // AD_ITEMS
    rng = np.random.default_rng(seed)
    q = np.arange(n, dtype=np.int64)
    block = q // AD_ITEMS
    out = {"empty": q[:0]}
    if n < 1:
        return out
    out["first_pixel"] = q[:1]
    out["last_pixel"] = q[-1:]
    out["all"] = q
    if n >= 2:
        out["first_and_last"] = q[[0, -1]]
    for m in LIST_SIZES:
        if m <= n:
            out[f"first_{m}"] = q[:m]
            out[f"last_{m}"] = q[n - m:]
    if n >= AD_ITEMS:
        out["mod1024_is_0"] = q[q % AD_ITEMS == 0]
        out["mod1024_is_1023"] = q[q % AD_ITEMS == AD_ITEMS - 1]
    if n >= 64:
        out["mod64_is_63"] = q[q % 64 == 63]
    if nb >= 2:
        out["all_but_block_0"] = q[block != 0]
        first = np.arange(nb, dtype=np.int64) * AD_ITEMS
        size = np.minimum(AD_ITEMS, n - first)
        out["one_per_block"] = first + rng.integers(0, size)
    if nb > SCAN_CHUNK + 1:
        out["block_255"] = q[block == SCAN_CHUNK - 1]
        out["block_256"] = q[block == SCAN_CHUNK]
        out["blocks_255_and_256"] = q[(block == SCAN_CHUNK - 1) | (block == SCAN_CHUNK)]
        out["blocks_from_256"] = q[block >= SCAN_CHUNK]
    for name, d in (("random_half", 0.5), ("random_hundredth", 0.01)):
        k = _random_size(n, d)
        if k >= 1:
            out[name] = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int64)
    out["random_three"] = np.sort(rng.choice(n, size=min(3, n), replace=False)).astype(np.int64)
    return out
