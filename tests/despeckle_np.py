"""The outlier filter of include/hrt.h ("despeckle") restated in numpy float32 from the header's words: the same
operations in the same order, one IEEE fp32 rounding each, vectorised over the pixels with a Python loop over the window in the header's
order (dy outer, dx inner).  The yardstick is read off a sorted stack of the window's luminances.  It shares nothing with
csrc/hrt_despeckle.hip; tests/test_gpu_despeckle.py requires the kernels to give its bits, tests/test_despeckle_cpu.py checks its
properties and decides the quality test on it."""
import numpy as np

F = np.float32
DEFAULTS = {"radius": 1, "rank": 2, "ratio": 2.0, "gate_z": 2.0, "repair_invalid": 1}


def lum(r, g, b):
    return F(0.2126) * r + F(0.7152) * g + F(0.0722) * b


def _window(radius):
    return [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]


def _shifted(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx] where that is inside the film, `fill` elsewhere"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H + min(0, -dy))
    xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W + min(0, -dx))
    b[yd, xd] = a[ys, xs]
    return b


def despeckle(rgb, var=None, radius=1, rank=2, ratio=2.0, gate_z=2.0, repair_invalid=1):
    """rgb [H, W, 3], var [H, W] or None -> (out [H, W, 3], map [H, W])"""
    assert radius in (1, 2) and 1 <= rank <= 4 and ratio > 1 and gate_z >= 0 and repair_invalid in (0, 1)
    c = np.ascontiguousarray(rgb, F)
    H, W = c.shape[:2]
    ratio, gate_z = F(ratio), F(gate_z)
    with np.errstate(all="ignore"):
        # 1. validity and luminance
        l = lum(c[..., 0], c[..., 1], c[..., 2]).astype(F)
        valid = np.isfinite(c).all(axis=-1) & np.isfinite(l)
        # 2. the yardstick: the rank-th largest luminance of the window's valid pixels, the centre left out
        lv = np.where(valid, l, F(-np.inf)).astype(F)
        stack = np.stack([_shifted(lv, dx, dy, F(-np.inf)) for dx, dy in _window(radius) if (dx, dy) != (0, 0)], axis=-1)
        others = np.stack([_shifted(valid, dx, dy, False) for dx, dy in _window(radius) if (dx, dy) != (0, 0)], axis=-1).sum(axis=-1)
        ref = (-np.sort(-stack, axis=-1))[..., rank - 1].astype(F)
        # 3. the outlier test
        outlier = valid & (others >= rank) & (l > 0) & (ref >= 0) & (l > ratio * ref)
        if var is not None and gate_z > 0:
            v = np.ascontiguousarray(var, F)
            assert v.shape == (H, W)
            outlier &= gate_z * np.sqrt(np.where(v > 0, v, F(0)).astype(F)) >= l - ref
        # 4. the kept part and the shares
        s = (ref / l).astype(F)
        n = (others + 1).astype(F)
        kept_o = (c * s[..., None]).astype(F)
        share_o = ((c - kept_o) / n[..., None]).astype(F)
        kept = np.where(outlier[..., None], kept_o, c).astype(F)
        share = np.where(outlier[..., None], share_o, F(0)).astype(F)
        # 5. the output
        out = kept.copy()
        total = np.zeros_like(c)
        count = np.zeros((H, W), np.int32)
        cz = np.where(valid[..., None], c, F(0)).astype(F)
        for dx, dy in _window(radius):
            vq = _shifted(valid, dx, dy, False)
            sq = _shifted(share, dx, dy, F(0))
            out = np.where(vq[..., None], out + sq, out).astype(F)
            cq = _shifted(cz, dx, dy, F(0))
            total = np.where(vq[..., None], total + cq, total).astype(F)
            count += vq
        repaired = ~valid & (count > 0) & bool(repair_invalid)
        mean = (total / count.astype(F)[..., None]).astype(F)
        out = np.where(valid[..., None], out, np.where(repaired[..., None], mean, c)).astype(F)
        # 6. the map
        dmap = np.where(outlier, F(1) - s, np.where(repaired, F(-1), F(0))).astype(F)
    return out, dmap
