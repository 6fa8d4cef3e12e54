"""tests/adaptive_np.py against itself on small arrays: the active sets are what their names say, the crafted buffers activate
exactly S and nothing else, and the expected buffers change nothing outside S (the GPU side is
tests/test_gpu_adaptive_sparse.py)."""
import numpy as np
import pytest

from tests import adaptive_np as ad

SIZES = [1, 2, 3, 15, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1073, 2048, 2049, 37 * 8, 5000,
         256 * 1024, 257 * 1024, 257 * 1024 + 1, 258 * 1024, 520 * 512]


@pytest.mark.parametrize("n", SIZES)
def test_patterns_are_subsets_of_the_promised_size(n):
    sets = ad.patterns(n, 3)
    sizes = ad.pattern_sizes(n)
    assert set(sets) == set(sizes)
    assert {"empty", "first_pixel", "last_pixel", "all", "first_1", "last_1", "random_three"} <= set(sets)
    for name, s in sets.items():
        assert s.dtype == np.int64 and s.ndim == 1, name
        assert (np.diff(s) > 0).all(), name                     # sorted, no duplicate
        assert s.size == 0 or (s[0] >= 0 and s[-1] < n), name
        assert s.size == sizes[name], name
    assert sets["all"].size == n and sets["first_pixel"][0] == 0 and sets["last_pixel"][0] == n - 1
    # the same seed gives the same sets, another one other random sets
    again = ad.patterns(n, 3)
    assert all(np.array_equal(sets[k], again[k]) for k in sets)
    if n >= 5000:
        assert not np.array_equal(sets["random_half"], ad.patterns(n, 4)["random_half"])


def test_patterns_say_what_they_mean():
    n = 520 * 512
    sets = ad.patterns(n, 0)
    nb = n // ad.AD_ITEMS
    assert nb == 260
    for m in ad.LIST_SIZES:
        assert np.array_equal(sets[f"first_{m}"], np.arange(m)) and np.array_equal(sets[f"last_{m}"], np.arange(n - m, n))
    assert (sets["mod1024_is_0"] % 1024 == 0).all() and (sets["mod1024_is_1023"] % 1024 == 1023).all() and (sets["mod64_is_63"] % 64 == 63).all()
    assert np.array_equal(np.unique(sets["block_255"] // 1024), [255]) and np.array_equal(np.unique(sets["block_256"] // 1024), [256])
    assert np.array_equal(np.unique(sets["blocks_255_and_256"] // 1024), [255, 256])
    assert np.array_equal(np.unique(sets["blocks_from_256"] // 1024), np.arange(256, nb))
    assert np.array_equal(np.unique(sets["all_but_block_0"] // 1024), np.arange(1, nb))
    assert np.array_equal(sets["one_per_block"] // 1024, np.arange(nb))
    # a film with a partial last block: its one pixel per block stays inside it, and the block sets need whole blocks 255 and 256
    sets = ad.patterns(1073, 0)
    assert np.array_equal(sets["one_per_block"] // 1024, [0, 1]) and sets["one_per_block"][1] < 1073
    assert "block_255" not in sets and "block_255" not in ad.patterns(257 * 1024, 0) and "block_255" in ad.patterns(257 * 1024 + 1, 0)
    assert set(ad.patterns(0, 0)) == {"empty"}


def _running(rows, W, spp, seed):
    rng = np.random.default_rng(seed)
    rad = rng.random((spp, rows, W, 3)).astype(np.float32) * np.float32(3.0)
    return rad, ad.sum_prefix(rad), ad.y2_prefix(rad)


@pytest.mark.parametrize("done", [2, 3, 4, 8])
@pytest.mark.parametrize("rows,W", [(1, 1), (3, 5), (29, 37)])
def test_crafted_activates_exactly_S_and_expect_leaves_the_rest_alone(rows, W, done):
    n = rows * W
    rad, prefix, y2 = _running(rows, W, done + 3, 1)
    for name, idx in ad.patterns(n, 9).items():
        S = ad.as_mask(idx, (rows, W))
        assert S.sum() == idx.size
        inputs = ad.crafted(prefix[done], y2[done], idx, done, seed=5)
        sums, sq, count = inputs
        assert sums.dtype == np.float32 and sq.dtype == np.float32 and count.dtype == np.int32
        assert sums.shape == (rows, W, 3) and sq.shape == count.shape == (rows, W)
        assert all(a.flags["C_CONTIGUOUS"] for a in inputs)
        # `done` in S and nowhere else; the rest from the five values, all of them when there is room
        assert np.array_equal(count == done, S), name
        assert set(count[~S].tolist()) <= set(ad.other_counts(done).tolist())
        if (~S).sum() >= 5:
            assert set(count[~S].tolist()) == set(ad.other_counts(done).tolist()), name
        assert ad.same_bits(sums[S], prefix[done][S]) and ad.same_bits(sq[S], y2[done][S])
        if (~S).any():
            assert np.isnan(sums[~S]).any() and np.isnan(sq[~S]).any(), name
        assert not np.isnan(sums[S]).any() and not np.isnan(sq[S]).any()
        # seeded
        assert all(ad.same_bits(a, b) for a, b in zip(inputs, ad.crafted(prefix[done], y2[done], S, done, seed=5)))
        # expect: the running sums after done + 3 in S, the inputs' bits (NaNs included) elsewhere, inputs not written to
        keep = [a.copy() for a in inputs]
        want = ad.expect(inputs, prefix[done + 3], y2[done + 3], idx, done, 3)
        assert all(ad.same_bits(a, b) for a, b in zip(inputs, keep))
        for w, i in zip(want, inputs):
            assert ad.same_bits(w[~S], i[~S]), name
        assert ad.same_bits(want[0][S], prefix[done + 3][S]) and ad.same_bits(want[1][S], y2[done + 3][S])
        assert (want[2][S] == done + 3).all()


def test_the_running_sums_are_float32_in_sample_order():
    rad = np.array([[[1e8, 1.0, 0.5]], [[1.0, 1e8, 0.25]], [[-1e8, 3.0, 0.125]]], np.float32)        # [3 samples, 1 pixel, rgb]
    p = ad.sum_prefix(rad)
    assert p.dtype == np.float32 and p.shape == (4, 1, 3)
    assert p[3, 0, 0] == np.float32(np.float32(np.float32(1e8) + np.float32(1.0)) + np.float32(-1e8)) == 0.0       # not the exact sum, 1
    assert p[3, 0, 2] == 0.875
    y = [np.float32(np.float32(np.float32(0.2126) * r + np.float32(0.7152) * g) + np.float32(0.0722) * b) for r, g, b in rad[:, 0]]
    assert np.array_equal(ad.luma(rad)[:, 0], np.array(y, np.float32))
    q = ad.y2_prefix(rad)
    assert q.dtype == np.float32 and q.shape == (4, 1) and q[0, 0] == 0
    acc = np.float32(0)
    for s in range(3):
        acc = np.float32(acc + np.float32(y[s] * y[s]))
        assert q[s + 1, 0] == acc
    assert not ad.same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    nan = np.array([np.nan], np.float32)
    assert ad.same_bits(nan, nan.copy())
