"""The develop stage of include/hrt.h ("develop") restated in numpy from the header's words: float32 operations in the
header's order, one IEEE rounding each, vectorised over the pixels with Python loops over the taps in the header's order (j outer, i
inner) and over the levels; the meter's walk over the 2048 bins is float64 and sequential, b ascending.  It shares nothing with
csrc/hrt_develop.hip; tests/test_gpu_develop.py requires the kernels to give its bits, tests/test_develop_cpu.py checks its properties."""
import numpy as np

F = np.float32
BINS = 2048
NONE, MANUAL, AUTO = 0, 1, 2
DEFAULTS = {"bloom_levels": 0, "bloom_strength": 0.05, "exposure_mode": 0, "exposure_ev": 0.0, "key": 0.18, "meter_low": 0.10, "meter_high": 0.90,
            "meter_floor": 2.0 ** -16, "ev_min": -16.0, "ev_max": 16.0}
TAP = (F(0.125), F(0.375), F(0.375), F(0.125))
MID = (0.0874628412503394, 0.2479275134435855, 0.3923174227787603, 0.5235619560570128,
       0.6438561897747247, 0.7548875021634686, 0.8579809951275721, 0.9541963103868752)


def lum(r, g, b):
    return F(0.2126) * r + F(0.7152) * g + F(0.0722) * b


def level_sizes(W, H, levels):
    """[(w, h)] of levels 1 .. L: halved, rounding up, while the larger side is above 1, `levels` at the most"""
    sizes = []
    while len(sizes) < levels and max(W, H) > 1:
        W, H = (W + 1) // 2, (H + 1) // 2
        sizes.append((W, H))
    return sizes


def down(D):
    h, w = D.shape[:2]
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    out = np.zeros((h2, w2, 3), F)
    for j in range(4):
        ys = np.clip(2 * np.arange(h2) - 1 + j, 0, h - 1)
        for i in range(4):
            xs = np.clip(2 * np.arange(w2) - 1 + i, 0, w - 1)
            out = out + D[ys][:, xs] * F(TAP[j] * TAP[i])
    return out


def up(C, wf, hf):
    h, w = C.shape[:2]
    x, y = np.arange(wf), np.arange(hf)
    cx, cy = x >> 1, y >> 1
    nx = np.clip(cx + np.where(x & 1, 1, -1), 0, w - 1)
    ny = np.clip(cy + np.where(y & 1, 1, -1), 0, h - 1)
    return C[cy][:, cx] * F(0.5625) + C[cy][:, nx] * F(0.1875) + C[ny][:, cx] * F(0.1875) + C[ny][:, nx] * F(0.0625)


def bloom(rgb, levels, strength):
    """-> (m, L): the film after steps 1 .. 5, the effective level count"""
    rgb = np.ascontiguousarray(rgb, F)
    H, W = rgb.shape[:2]
    sizes = level_sizes(W, H, levels)
    L = len(sizes)
    s = F(strength)
    if L == 0 or s == 0:
        return rgb.copy(), L
    valid = np.isfinite(rgb).all(axis=-1)
    with np.errstate(all="ignore"):
        D = [np.where(valid[..., None], rgb, F(0))]
        for _ in range(L):
            D.append(down(D[-1]))
        E = D[L]
        for k in range(L - 1, 0, -1):
            E = D[k] + up(E, D[k].shape[1], D[k].shape[0])
        B = up(E, W, H) / F(L)
        m = rgb * (F(1.0) - s) + B * s
    return np.where(valid[..., None], m, rgb), L


def histogram(m, meter_floor):
    """the meter's 2048 exact bin counts of the film m"""
    with np.errstate(all="ignore"):
        valid = np.isfinite(m).all(axis=-1)
        l = lum(m[..., 0], m[..., 1], m[..., 2])
        metered = valid & np.isfinite(l) & (l >= F(meter_floor))
    bins = np.ascontiguousarray(l[metered], F).view(np.uint32) >> 20
    return np.bincount(bins, minlength=BINS).astype(np.uint32)


def meter(hist, key=0.18, meter_low=0.10, meter_high=0.90, ev_min=-16.0, ev_max=16.0):
    """-> (scale as float32, mean_ev as float64, N)"""
    N = int(hist.sum())
    if N == 0:
        return F(1.0), 0.0, 0
    lo, hi = np.float64(F(meter_low)) * N, np.float64(F(meter_high)) * N
    num = den = np.float64(0.0)
    C = 0
    for b in range(BINS):
        n = int(hist[b])
        o = max(np.float64(0.0), min(np.float64(C + n), hi) - max(np.float64(C), lo))
        ev = np.float64((b >> 3) - 127) + np.float64(MID[b & 7])
        num = num + o * ev
        den = den + o
        C += n
    mean_ev = min(max(num / den, np.float64(F(ev_min))), np.float64(F(ev_max)))
    return F(np.float64(F(key)) * np.exp2(-mean_ev)), float(mean_ev), N


def develop(rgb, scale=None, **params):
    """-> (out, m, info, hist): info = {"mean_ev", "scale", "metered", "levels"}.  `scale`: use this one instead of the restatement's own
    (the header pins the film to m * the scale the call reports, and the scale itself to one ulp)."""
    p = dict(DEFAULTS)
    for k in params:
        if k not in p:
            raise TypeError(k)
    p.update(params)
    rgb = np.ascontiguousarray(rgb, F)
    src_valid = np.isfinite(rgb).all(axis=-1)
    m, L = bloom(rgb, p["bloom_levels"], p["bloom_strength"])
    hist = np.zeros(BINS, np.uint32)
    info = {"mean_ev": 0.0, "scale": F(1.0), "metered": 0, "levels": L}
    if p["exposure_mode"] == NONE:
        return m, m, info, hist
    if p["exposure_mode"] == MANUAL:
        info["scale"] = F(np.exp2(np.float64(F(p["exposure_ev"]))))
    else:
        hist = histogram(m, p["meter_floor"])
        info["scale"], info["mean_ev"], info["metered"] = meter(hist, p["key"], p["meter_low"], p["meter_high"], p["ev_min"], p["ev_max"])
    with np.errstate(all="ignore"):
        out = np.where(src_valid[..., None], m * F(info["scale"] if scale is None else scale), m)
    return out, m, info, hist
