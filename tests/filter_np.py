"""The reconstruction filter of include/hrt.h ("reconstruction filter") restated in numpy float32 from the header's
words: the same operations in the same order, one IEEE fp32 rounding each, vectorised over the pixels with Python loops over the samples
and over the window in the header's order (qy outer, qx inner).  The jitters come from tests/f64_reference.py's and
tests/stratified_np.py's `draw`.  It shares nothing with csrc/hrt_filter.hip; tests/test_gpu_filter.py requires the kernels to give its
bits, tests/test_filter_cpu.py checks its properties.

The window visited here is 7 x 7 whatever the radius: wider than any counting tap (the header: "any window that holds every counting
tap gives the same bits"), so the kernels' choice of a narrower one is tested, not assumed."""
import numpy as np

from tests import f64_reference as ref
from tests import stratified_np as strat

F = np.float32
TENT, BSPLINE, MITCHELL = 0, 1, 2
KINDS = {"tent": TENT, "bspline": BSPLINE, "mitchell": MITCHELL}
DEFAULT_RADIUS = {TENT: 1.0, BSPLINE: 2.0, MITCHELL: 2.0}
RNG_JITTER = 0
HALF_WIDTH = 3
C16_3, C7_3, C32_3 = F(16.0 / 3.0), F(7.0 / 3.0), F(32.0 / 3.0)      # the nearest floats


def resolve(kind, radius):
    kind = KINDS.get(kind, kind)
    assert kind in (TENT, BSPLINE, MITCHELL)
    R = F(DEFAULT_RADIUS[kind] if radius <= 0 else radius)
    assert F(0.5) <= R <= F(2.5)
    return kind, R


def kernel(kind, t):
    """k(t) for t in [0, 1), float32 in, float32 out"""
    t = np.asarray(t, F)
    if kind == TENT:
        return (F(1) - t).astype(F)
    x = (t + t).astype(F)
    if kind == BSPLINE:
        a = F(3) * x - F(6); a = a * x; a = a * x; a = a + F(4)
        u = F(2) - x; b = (u * u) * u
    else:
        a = F(7) * x - F(12); a = a * x; a = a * x; a = a + C16_3
        b = -C7_3 * x + F(12); b = b * x - F(20); b = b * x + C32_3
    return (np.where(x < F(1), a, b).astype(F) / F(6)).astype(F)


def jitters(W, rect, samples, seed=0, stratified=False):
    """(jx, jy) [S, h, w] float32 of the samples `samples` (a sequence of S indices) of the pixels of rect = (x0, y0, w, h) of a film W wide"""
    x0, y0, w, h = rect
    py, px = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
    pixel = (py * W + px).astype(np.uint64)[None]
    sample = np.asarray(list(samples), np.uint64)[:, None, None]
    draw = strat.draw if stratified else ref.draw
    u = draw(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, np.broadcast_to(pixel, (sample.shape[0], h, w)), np.broadcast_to(sample, (sample.shape[0], h, w)),
             0, RNG_JITTER)
    to01 = lambda word: (np.asarray(word, np.uint32) >> np.uint32(8)).astype(F) * F(2.0 ** -24)      # noqa: E731
    return to01(u[0]), to01(u[1])


def _shifted(a, ox, oy, fill):
    """a [S, h, w, ...]: b[:, y, x] = a[:, y + oy, x + ox] where that is inside the rectangle, `fill` elsewhere"""
    H, W = a.shape[1:3]
    b = np.full_like(a, fill)
    if abs(ox) >= W or abs(oy) >= H:
        return b
    ys, yd = slice(max(0, oy), H + min(0, oy)), slice(max(0, -oy), H + min(0, -oy))
    xs, xd = slice(max(0, ox), W + min(0, ox)), slice(max(0, -ox), W + min(0, -ox))
    b[:, yd, xd] = a[:, ys, xs]
    return b


def taps(kind, R, jx, jy, half_width=HALF_WIDTH):
    """the taps of every sample in the header's order within a sample: a list of (ox, oy, counts [S, h, w] bool, w [S, h, w] float32); only
    the arithmetic of a tap is vectorised over the samples, the sums below still take sample after sample"""
    out = []
    for oy in range(-half_width, half_width + 1):
        for ox in range(-half_width, half_width + 1):
            qjx, qjy = _shifted(jx, ox, oy, F(np.nan)), _shifted(jy, ox, oy, F(np.nan))
            dx = (F(ox) + qjx) - F(0.5)            # qx - px = ox
            dy = (F(-oy) + qjy) - F(0.5)           # py - qy = -oy
            with np.errstate(invalid="ignore"):
                tx, ty = (np.abs(dx) / R).astype(F), (np.abs(dy) / R).astype(F)
                counts = (tx < F(1)) & (ty < F(1))
                if counts.any():
                    out.append((ox, oy, counts, (kernel(kind, tx) * kernel(kind, ty)).astype(F)))
    return out


def accumulate(rad, kind, radius, W, rect, seed=0, stratified=False, sample_first=0, acc=None, half_width=HALF_WIDTH):
    """acc [h, w, 3] after the samples rad [S, h, w, 3] = samples sample_first .. sample_first + S - 1 have been added"""
    kind, R = resolve(kind, radius)
    rad = np.ascontiguousarray(rad, F)
    S, h, w = rad.shape[:3]
    assert (w, h) == tuple(rect[2:])
    assert sample_first == 0 or acc is not None
    acc = np.zeros((h, w, 3), F) if sample_first == 0 else np.array(acc, F)
    with np.errstate(all="ignore"):
        jx, jy = jitters(W, rect, range(sample_first, sample_first + S), seed, stratified)
        tp = [(counts, wt, _shifted(rad, ox, oy, F(0))) for ox, oy, counts, wt in taps(kind, R, jx, jy, half_width)]
        for k in range(S):
            for counts, wt, v in tp:
                if counts[k].any():
                    acc = np.where(counts[k][..., None], acc + wt[k][..., None] * v[k], acc).astype(F)
    return acc


def weight_sums(samples, kind, radius, W, rect, seed=0, stratified=False, half_width=HALF_WIDTH):
    """Wsum [h, w] over all samples [0, samples)"""
    kind, R = resolve(kind, radius)
    wsum = np.zeros((rect[3], rect[2]), F)
    with np.errstate(all="ignore"):
        jx, jy = jitters(W, rect, range(samples), seed, stratified)
        tp = taps(kind, R, jx, jy, half_width)
        for s in range(samples):
            for _, _, counts, wt in tp:
                if counts[s].any():
                    wsum = np.where(counts[s], wsum + wt[s], wsum).astype(F)
    return wsum


def finish(acc, wsum):
    with np.errstate(all="ignore"):
        out = np.where(wsum[..., None] > F(0), acc / wsum[..., None], F(0)).astype(F)
        return np.where(out < F(0), F(0), out).astype(F)


def filter_samples(rad, kind, radius=0.0, W=None, rect=None, seed=0, stratified=False, half_width=HALF_WIDTH):
    """rad [S, h, w, 3] -> the finished film [h, w, 3] (hrt_filter_samples)"""
    rad = np.ascontiguousarray(rad, F)
    S, h, w = rad.shape[:3]
    rect = (0, 0, w, h) if rect is None else tuple(rect)
    W = w if W is None else W
    acc = accumulate(rad, kind, radius, W, rect, seed, stratified, half_width=half_width)
    return finish(acc, weight_sums(S, kind, radius, W, rect, seed, stratified, half_width))
