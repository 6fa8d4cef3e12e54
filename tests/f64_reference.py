"""Float64 restatement of the camera, the miss branch, the textures and ConstantMedium, written from the reference's formulas
alone (camera.h:9-39, main.cpp:47-58 and 115-121, texture.cpp:17-28 / 53-97, aarect.cpp, sphere.cpp:4-18 and 20-46,
constantMedium.cpp:8-31) plus the counter layout of csrc/hrt_rng.h.  numpy only: nothing here is shared with the oracle, the
device header or the host library, so a misreading common to those cannot hide from it.

fp32 moves every continuous coordinate by a few ulps.  Comparisons therefore use an ambiguity band: an input coordinate x is
ambiguous when the index function takes different values at x - delta and x + delta; outside the band the product must give the
float64 index exactly, inside it one of the two neighbours.  delta is BAND_ULPS * 2^-24 times the magnitude the coordinate was
computed from (see each *_delta helper); tests assert that the band holds fewer than 2 % of the samples, so a loose band cannot
hide a real error."""
import numpy as np

BAND_ULPS = 64
EPS = BAND_ULPS * 2.0 ** -24          # relative width of the ambiguity band

# hrt_rng.h rng_purpose
RNG_JITTER, RNG_SCATTER, RNG_MEDIUM, RNG_BALL, RNG_BUILD, RNG_LENS = range(6)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11), vectorised: every argument broadcasts; returns 4 uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(a, dtype=np.uint64) & _LO for a in (c0, c1, c2, c3, k0, k1)])
    c0, c1, c2, c3, k0, k1 = (a.copy() for a in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ k0
        n2 = (p0 >> _S32) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & _LO, n2, p0 & _LO
        k0 = (k0 + _W0) & _LO
        k1 = (k1 + _W1) & _LO
    return tuple(a.astype(np.uint32) for a in (c0, c1, c2, c3))


def draw(seed_lo, seed_hi, pixel, sample, bounce, purpose, aux=0):
    """hrt_rng.h: key (seed_lo, seed_hi), counter (pixel, sample, bounce, purpose | aux << 8)."""
    word3 = np.uint64(purpose) | (np.asarray(aux, dtype=np.uint64) << np.uint64(8))
    return philox4x32_10(pixel, sample, bounce, word3, seed_lo, seed_hi)


def u01(u):
    """(u >> 8) * 2^-24: exact in float64."""
    return (np.asarray(u, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------ camera (camera.h:9-39, main.cpp:115-121)
def camera(look_from, look_at, up, vfov_deg, aspect, aperture=0.0, focus=1.0):
    look_from, look_at, up = (np.asarray(a, np.float64) for a in (look_from, look_at, up))
    h = np.tan(np.radians(vfov_deg) / 2)
    vh = 2.0 * h
    vw = aspect * vh
    w = _normalize(look_from - look_at)
    u = _normalize(np.cross(up, w))
    v = np.cross(w, u)
    hor = focus * vw * u
    ver = focus * vh * v
    return dict(origin=look_from, horizontal=hor, vertical=ver, lower_left=look_from - hor / 2 - ver / 2 - focus * w,
                u=u, v=v, lens_radius=aperture / 2.0)


def primary_rays(cam, W, H, px, py, sample, seed_lo, seed_hi, thin_lens=False):
    """Sample `sample` of global pixel (px, py): x = px, y = H - py (Q-10), denominators W-1 and H-1, jitter words x, y of
    (pixel, sample, 0, RNG_JITTER); with the thin lens, circularRand(lensRadius) from word x of (pixel, sample, 0, RNG_LENS).
    -> (origins, directions), float64, shape px.shape + (3,)."""
    px, py = np.broadcast_arrays(np.asarray(px, np.int64), np.asarray(py, np.int64))
    pix = (py * W + px).astype(np.uint64)
    j = draw(seed_lo, seed_hi, pix, sample, 0, RNG_JITTER)
    s = (px + u01(j[0])) / (W - 1)
    t = (H - py + u01(j[1])) / (H - 1)
    offset = np.zeros(px.shape + (3,))
    if thin_lens:
        a = u01(draw(seed_lo, seed_hi, pix, sample, 0, RNG_LENS)[0]) * (2 * np.pi)
        r = cam["lens_radius"]
        offset = (r * np.cos(a))[..., None] * cam["u"] + (r * np.sin(a))[..., None] * cam["v"]
    o = cam["origin"] + offset
    d = cam["lower_left"] + s[..., None] * cam["horizontal"] + t[..., None] * cam["vertical"] - o
    return o, d


# ------------------------------------------------------------------ miss branch (main.cpp:47-58) and EnvironmentMap (texture.cpp:76-97)
def miss_uv(d):
    n = _normalize(np.asarray(d, np.float64))
    u = np.arctan2(n[..., 2], n[..., 0]) / (2 * np.pi) + 0.5
    v = np.arccos(np.clip(n[..., 1], -1, 1)) / np.pi
    return u, v


def miss_uv_delta(d):
    """Band of miss_uv: a unit direction carries ~EPS of absolute error; atan2 and acos magnify it by 1 / r_xz."""
    n = _normalize(np.asarray(d, np.float64))
    r = np.maximum(np.hypot(n[..., 0], n[..., 2]), 1e-300)
    return EPS / (2 * np.pi * r), EPS / (np.pi * r)


def env_index(u, n):
    """int(clamp(u, 0, 1) * (n - 1) + 0.5)."""
    return np.floor(np.clip(u, 0.0, 1.0) * (n - 1) + 0.5).astype(np.int64)


# ------------------------------------------------------------------ ImageTexture (texture.cpp:53-74)
def image_i(u, width):
    return np.minimum(np.floor(np.clip(np.nan_to_num(u), 0.0, 1.0) * width).astype(np.int64), width - 1)


def image_j(v, height):
    """v flipped to image rows: int((1 - clamp(v, 0, 1)) * height), clamped to height - 1."""
    return np.minimum(np.floor((1.0 - np.clip(np.nan_to_num(v), 0.0, 1.0)) * height).astype(np.int64), height - 1)


# ------------------------------------------------------------------ UV mappings and CheckeredTexture
def rect_uv(p, a_axis, b_axis, a0, a1, b0, b1):
    """aarect.cpp: u = (a - a0) / (a1 - a0), v = (b - b0) / (b1 - b0)."""
    return (p[..., a_axis] - a0) / (a1 - a0), (p[..., b_axis] - b0) / (b1 - b0)


def sphere_uv(n):
    """sphere.cpp:4-18 for the outward unit normal n: u = (atan2(-z, x) + pi) / 2pi, v = acos(-y) / pi."""
    u = (np.arctan2(-n[..., 2], n[..., 0]) + np.pi) / (2 * np.pi)
    v = np.arccos(np.clip(-n[..., 1], -1, 1)) / np.pi
    return u, v


def checker_odd(p):
    """texture.cpp:17-28: odd when sin(10x) sin(10y) sin(10z) < 0; sines == 0 is even."""
    s = np.sin(10 * p[..., 0]) * np.sin(10 * p[..., 1]) * np.sin(10 * p[..., 2])
    return s < 0


def checker_ambiguous(p, scale):
    """A factor sin(10 p_c) within 10 * EPS * scale of zero (scale: the magnitude p was computed from)."""
    return (np.abs(np.sin(10 * p)) < 10 * EPS * np.asarray(scale)[..., None]).any(axis=-1)


# ------------------------------------------------------------------ ray vs. primitives, float64
def rect_hit(o, d, axis, a0, a1, b0, b1, k):
    """(t, p, hit) of an axis-aligned rect (axis = the constant axis), no t range."""
    ab = [i for i in range(3) if i != axis]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (k - o[..., axis]) / d[..., axis]
    p = o + t[..., None] * d
    hit = np.isfinite(t) & (t > 0) & (p[..., ab[0]] >= a0) & (p[..., ab[0]] <= a1) & (p[..., ab[1]] >= b0) & (p[..., ab[1]] <= b1)
    return t, p, hit


def sphere_roots(o, d, c, r):
    """(t_near, t_far, closest-approach distance of the line to the centre)."""
    oc = o - np.asarray(c, np.float64)
    a = (d * d).sum(-1)
    hb = (oc * d).sum(-1)
    cc = (oc * oc).sum(-1) - r * r
    disc = hb * hb - a * cc
    sq = np.sqrt(np.maximum(disc, 0))
    dist = np.sqrt(np.maximum((oc * oc).sum(-1) - hb * hb / a, 0))
    t0, t1 = (-hb - sq) / a, (-hb + sq) / a
    t0 = np.where(disc >= 0, t0, np.nan)
    t1 = np.where(disc >= 0, t1, np.nan)
    return t0, t1, dist


def sphere_root_error(o, d, c, r):
    """fp32 resolution of sphere.cpp's roots: (-half_b -+ sqrt(disc)) / a, where disc = half_b^2 - a c cancels near a tangent.
    EPS * (half_b^2 + |a c|) / (a sqrt(disc)) + EPS * |half_b| / a."""
    oc = o - np.asarray(c, np.float64)
    a = (d * d).sum(-1)
    hb = (oc * d).sum(-1)
    cc = (oc * oc).sum(-1) - r * r
    disc = np.maximum(hb * hb - a * cc, 1e-300)
    return EPS * (hb * hb + np.abs(a * cc)) / (a * np.sqrt(disc)) + EPS * np.abs(hb) / a


def box_slabs(o, d, bmin, bmax):
    """(t_near, t_far) of the slab test; t_near > t_far: no intersection of the line."""
    bmin, bmax = np.asarray(bmin, np.float64), np.asarray(bmax, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta = (bmin - o) / d
        tb = (bmax - o) / d
    lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
    return np.nanmax(lo, axis=-1), np.nanmin(hi, axis=-1)


# ------------------------------------------------------------------ ConstantMedium (constantMedium.cpp:8-31)
def _extent(geom):
    """Largest coordinate magnitude of a boundary ((centre, radius) or (min, max)): the scale of its fp32 arithmetic."""
    return float(np.abs(np.hstack([np.ravel(np.asarray(g, np.float64)) for g in geom])).max())


def medium_boundary(kind, geom, o, d):
    """rec1 = boundary->hit(-inf, inf), rec2 = boundary->hit(rec1.t + 0.0001, inf).  -> (t1, t2, ok, ambiguous).
    A box is the six rects of box.h: the first face hit is the entry, the second one the exit, found only when the exit lies
    at least 1e-4 (in t) beyond the entry.  Ambiguous: the line grazes the boundary (tangent to the sphere, through an edge of
    the box) or the chord lies within the band of 1e-4."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    L = np.linalg.norm(d, axis=-1)
    scale = np.linalg.norm(o, axis=-1) + _extent(geom)
    if kind == "sphere":
        c, r = geom
        t1, t2, dist = sphere_roots(o, d, c, r)
        line = np.isfinite(t1)
        # a tangent's chord is 2 sqrt(2 r h) for a miss distance h: the band covers that chord's fp32 uncertainty
        graze = np.abs(dist - r) < EPS * scale
    else:
        bmin, bmax = np.asarray(geom[0], np.float64), np.asarray(geom[1], np.float64)
        t1, t2 = box_slabs(o, d, bmin, bmax)
        line = t1 <= t2
        graze = np.zeros(t1.shape, bool)
        for t in (t1, t2):     # an entry or exit point on an edge: two coordinates on the box's bounds
            p = o + t[..., None] * d
            near = (np.abs(p - bmin) < EPS * scale[..., None]) | (np.abs(p - bmax) < EPS * scale[..., None])
            graze |= line & (near.sum(-1) >= 2)
    with np.errstate(invalid="ignore"):
        reentry = line & (t2 >= t1 + 1e-4)
        band = line & (np.abs(t2 - t1 - 1e-4) < EPS * scale / L + 1e-4 * 2.0 ** -10)
    return t1, t2, reentry, graze | band


def medium_free_path(kind, geom, density, o, d, t_min, t_max, u):
    """t of the medium hit, NaN for no hit, float64, plus (t1 after the clamps, ambiguous).  u: the linearRand(0, 1) of the
    ray, i.e. u01(word x of (pixel, sample, bounce, RNG_MEDIUM | prim << 8))."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    t1, t2, ok, amb = medium_boundary(kind, geom, o, d)
    L = np.linalg.norm(d, axis=-1)
    scale = (np.linalg.norm(o, axis=-1) + _extent(geom)) / L
    t_max = np.broadcast_to(np.asarray(t_max, np.float64), t1.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(t1 < t_min, t_min, t1)
        b = np.where(t2 > t_max, t_max, t2)
        ok = ok & (a < b)
        amb |= np.abs(a - b) < EPS * scale
        a = np.maximum(a, 0.0)
        dist = (b - a) * L
        hd = (-1.0 / density) * np.log(u)
        amb |= ok & (np.abs(hd - dist) < EPS * (scale * L + hd))
        ok = ok & (hd <= dist)
        t = np.where(ok, a + hd / L, np.nan)
    return t, a, amb


# ------------------------------------------------------------------ the band rule
def band(f, x, delta):
    """(index at x, index at x - delta, index at x + delta, ambiguous) for a monotone index function f."""
    lo, hi = f(x - delta), f(x + delta)
    return f(x), lo, hi, lo != hi


def band_wrap(f, x, delta):
    """band() for a periodic coordinate in [0, 1] (the seam of atan2 at phi = +-pi): x +- delta taken modulo 1."""
    lo, hi = f(np.mod(x - delta, 1.0)), f(np.mod(x + delta, 1.0))
    return f(x), lo, hi, lo != hi
