"""numpy float64 restatement of HRT_FLAG_NEE_ENV's environment-map sampling table (hrt_device.h env_*): the cells of the
reference's nearest-texel lookup, their solid angles, the texel weights and the two CDFs, stored as fp32."""
import numpy as np

LUM = (0.2126, 0.7152, 0.0722)


def edges(n):
    """[lo, hi] of texel k of n along one axis of i = int(u (n - 1) + 0.5), as fractions of the axis"""
    if n <= 1:
        return np.zeros(1), np.ones(1)
    k = np.arange(n, dtype=np.float64)
    lo = np.where(k == 0, 0.0, (k - 0.5) / (n - 1))
    return lo, lo + np.where((k == 0) | (k == n - 1), 0.5, 1.0) / (n - 1)


def cells(W, H):
    """phi0, dphi [W] and theta0, theta1, dc [H] (dc = cos theta0 - cos theta1) in float64"""
    u0, u1 = edges(W)
    v0, v1 = edges(H)
    th0, th1 = np.pi * v0, np.pi * v1
    du = np.where((np.arange(W) == 0) | (np.arange(W) == W - 1), 0.5, 1.0) / max(1, W - 1) if W > 1 else np.ones(1)
    dv = np.where((np.arange(H) == 0) | (np.arange(H) == H - 1), 0.5, 1.0) / max(1, H - 1) if H > 1 else np.ones(1)
    return 2 * np.pi * (u0 - 0.5), 2 * np.pi * du, th0, th1, 2 * np.sin(0.5 * (np.pi * dv)) * np.sin(th0 + 0.5 * (np.pi * dv))


def solid_angles(W, H):
    _, dphi, _, _, dc = cells(W, H)
    return dphi[None, :] * dc[:, None]


def weights(tex):
    """lum x solid angle of every texel of tex [H, W, C >= 3]; 0 for a negative, NaN or infinite channel"""
    t = np.asarray(tex, np.float32)[..., :3]
    H, W = t.shape[:2]
    ok = np.all(np.isfinite(t) & (t >= 0), axis=-1)
    t64 = np.where(ok[..., None], t, 0).astype(np.float64)
    lum = LUM[0] * t64[..., 0] + LUM[1] * t64[..., 1] + LUM[2] * t64[..., 2]
    return np.where(ok, lum * solid_angles(W, H), 0.0)


def _cdf(w):
    """fp32 CDF (len(w) + 1 entries) of float64 weights, 0 first and 1 last; a total of 0 gives 0 everywhere but the last"""
    out = np.zeros(len(w) + 1, np.float32)
    tot = w.sum()
    if tot > 0 and np.isfinite(tot):
        out[1:] = (np.cumsum(w) / tot).astype(np.float32)
    out[-1] = 1.0
    return out


def table(tex):
    """(marginal [H + 1], conditional [H, W + 1]) fp32, or None when the map has no table"""
    w = weights(tex)
    rows = w.sum(axis=1)
    total = rows.sum()
    if not (total > 0 and np.isfinite(total)):
        return None
    return _cdf(rows), np.stack([_cdf(r) for r in w])


def cell_probs(marg, cond):
    """P(cell) = P_row P_col from differences of the stored fp32 CDFs (the arithmetic of env_cell_prob)"""
    return np.diff(marg)[:, None] * np.diff(cond, axis=1)


def directions(phi, cos_theta):
    phi, cos_theta = np.broadcast_arrays(phi, cos_theta)
    s = np.sqrt(np.maximum(0.0, 1.0 - cos_theta * cos_theta))
    return np.stack([s * np.cos(phi), cos_theta, s * np.sin(phi)], axis=-1)


def centre_directions(W, H):
    """[H, W, 3] float64 unit directions at the centre (in phi and cos theta) of every cell"""
    phi0, dphi, th0, _, dc = cells(W, H)
    phi = phi0 + 0.5 * dphi
    ct = np.cos(th0) - 0.5 * dc
    return directions(phi[None, :], ct[:, None])


def messy_map(rng, W, H):
    """a random HDR map with a zero row, a zero column and NaN, infinite and negative texels"""
    tex = rng.gamma(0.6, 1.0, size=(H, W, 3)).astype(np.float32)
    tex[rng.random((H, W)) < 0.2] *= 40.0
    tex[H // 3] = 0.0
    tex[:, W // 2] = 0.0
    bad = rng.integers(0, W * H, 12)
    vals = [np.nan, np.inf, -np.inf, -1.0]
    for k, b in enumerate(bad):
        tex[b // W, b % W, k % 3] = vals[k % 4]
    return tex
