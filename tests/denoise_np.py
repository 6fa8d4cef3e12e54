"""The guided denoiser of include/hrt.h ("guided denoiser") restated in numpy float32 from the header's words: the same
operations in the same order, one IEEE fp32 rounding each, vectorised over the pixels with a Python loop over the taps in the header's
order (dy outer, dx inner).  It shares nothing with csrc/hrt_denoise.hip; tests/test_gpu_denoise.py requires the kernels to give its bits,
tests/test_denoise_cpu.py checks its properties and decides the quality test on it."""
import numpy as np

F = np.float32
DEFAULTS = {"iterations": 5, "normal_squarings": 7, "sigma_l": 2.5, "sigma_z": 0.5, "albedo_floor": 0.01}
K5 = (F(0.375), F(0.25), F(0.0625))
B3 = (F(0.5), F(0.25))


def lum(r, g, b):
    return F(0.2126) * r + F(0.7152) * g + F(0.0722) * b


def _pos(x):
    """max(0, x) of the header: x > 0 ? x : 0"""
    return np.where(x > 0, x, F(0))


def _falloff(x):
    u = _pos(F(1) - x)
    return u * u


def _shift(a, ox, oy):
    """b[y, x] = a[y + oy, x + ox] where that is inside the film (elsewhere: unspecified, masked by `inside`)"""
    return np.roll(a, (-oy, -ox), axis=(0, 1))


def _inside(H, W, ox, oy):
    y, x = np.mgrid[0:H, 0:W]
    return (y + oy >= 0) & (y + oy < H) & (x + ox >= 0) & (x + ox < W)


def prepare(rgb, aov, var, albedo_floor):
    """-> e [H, W, 3], v [H, W] (None when var is None), nh [H, W, 3], z [H, W], af [H, W, 3], valid [H, W]"""
    rgb = np.ascontiguousarray(rgb, F)
    aov = np.ascontiguousarray(aov, F)
    fl = F(albedo_floor)
    a = aov[..., 0:3]
    af = np.where(a > fl, a, fl).astype(F)
    valid = np.isfinite(rgb).all(axis=-1)
    e = rgb / af
    n = aov[..., 4:7]
    d = n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2]
    inv = F(1) / np.sqrt(d)
    nh = np.where((d > 0)[..., None], n * inv[..., None], F(0)).astype(F)
    alpha, depth = aov[..., 3], aov[..., 7]
    z = np.where(alpha > 0, depth / alpha, F(0)).astype(F)
    v = None
    if var is not None:
        var = np.ascontiguousarray(var, F)
        ya = lum(af[..., 0], af[..., 1], af[..., 2])
        v = (np.where(var > 0, var, F(0)) / (ya * ya)).astype(F)
    return e.astype(F), v, nh, z, af, valid


def spatial_variance(e, valid):
    H, W = valid.shape
    l = lum(e[..., 0], e[..., 1], e[..., 2])
    s1, s2, n = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            use = _inside(H, W, dx, dy) & _shift(valid, dx, dy)
            lq = _shift(l, dx, dy)
            s1 = np.where(use, s1 + lq, s1)
            s2 = np.where(use, s2 + lq * lq, s2)
            n = np.where(use, n + F(1), n)
    m = s1 / n
    return _pos(s2 / n - m * m).astype(F)


def iteration(e, v, nh, z, valid, step, sigma_l, sigma_z, normal_squarings):
    H, W = valid.shape
    sigma_l, sigma_z = F(sigma_l), F(sigma_z)
    vs, gs = np.zeros((H, W), F), np.zeros((H, W), F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            use = _inside(H, W, dx, dy) & _shift(valid, dx, dy)
            g = B3[abs(dx)] * B3[abs(dy)]
            vs = np.where(use, vs + g * _shift(v, dx, dy), vs)
            gs = np.where(use, gs + g, gs)
    sd = np.sqrt(vs / gs)
    den_l = sigma_l * sd + F(1e-6)
    l = lum(e[..., 0], e[..., 1], e[..., 2])
    p_zero = (nh == 0).all(axis=-1)
    sums = np.zeros((H, W, 3), F)
    sw, sv = np.zeros((H, W), F), np.zeros((H, W), F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ox, oy = dx * step, dy * step
            use = _inside(H, W, ox, oy) & _shift(valid, ox, oy)
            if not use.any():
                continue
            eq, vq, nq, zq, lq = _shift(e, ox, oy), _shift(v, ox, oy), _shift(nh, ox, oy), _shift(z, ox, oy), _shift(l, ox, oy)
            h = K5[abs(dx)] * K5[abs(dy)]
            if dx == 0 and dy == 0:
                w = np.full((H, W), h, F)
            else:
                q_zero = (nq == 0).all(axis=-1)
                t = _pos(nh[..., 0] * nq[..., 0] + nh[..., 1] * nq[..., 1] + nh[..., 2] * nq[..., 2])
                for _ in range(normal_squarings):
                    t = t * t
                wn = np.where(p_zero & q_zero, F(1), np.where(p_zero | q_zero, F(0), t)).astype(F)
                wz = _falloff(np.abs(z - zq) / (sigma_z * np.where(z > zq, z, zq) + F(1e-6)))
                wl = _falloff(np.abs(l - lq) / den_l)
                w = h * wn * wz * wl
            sums = np.where(use[..., None], sums + w[..., None] * eq, sums)
            sw = np.where(use, sw + w, sw)
            sv = np.where(use, sv + (w * w) * vq, sv)
    e2 = sums / sw[..., None]
    v2 = sv / (sw * sw)
    e2 = np.where(valid[..., None], e2, e)
    v2 = np.where(valid, v2, v)
    return e2.astype(F), v2.astype(F)


def denoise(rgb, aov, var=None, **params):
    """[H, W, 3] linear film, [H, W, 8] feature buffer, optional [H, W] variance of the mean luminance -> the filtered film [H, W, 3]"""
    p = dict(DEFAULTS)
    p.update(params)
    rgb = np.ascontiguousarray(rgb, F)
    with np.errstate(all="ignore"):
        e, v, nh, z, af, valid = prepare(rgb, aov, var, p["albedo_floor"])
        if v is None:
            v = np.where(valid, spatial_variance(e, valid), F(0)).astype(F)
        for j in range(p["iterations"]):
            e, v = iteration(e, v, nh, z, valid, 1 << j, p["sigma_l"], p["sigma_z"], p["normal_squarings"])
        out = np.where(valid[..., None], e * af, rgb)
    return out.astype(F)


def variance_of_mean_luminance(sums, sq, count):
    """The `var` input from the buffers of an adaptive render (include/hrt.h): sums [H, W, 3] of the samples, sq [H, W] the sums of their
    squared luminances, count [H, W] -> max(0, (sq - n m m) / (n - 1)) / n with m = Y(sums) / n, in fp32."""
    n = count.astype(F)
    with np.errstate(all="ignore"):
        m = lum(sums[..., 0], sums[..., 1], sums[..., 2]) / n
        s = (sq - n * m * m) / (n - F(1))
        return (np.where(s > 0, s, F(0)) / n).astype(F)
