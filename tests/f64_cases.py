"""Scenes and rays whose exact answer tests/f64_reference.py predicts, and the checks of a renderer's output against that
prediction.  Shared by tests/test_f64_pins.py (oracle, device code on the CPU) and tests/test_gpu_f64_pins.py (HIP kernels):
each takes a `render(hs, cam, params, rect)` or `closest_hit(hs, params, o, d, t_min, t_max, pixel0)` of its implementation."""
import os

import numpy as np

from tests import f64_reference as F

SEED = (0x7F4A7C15 << 32) | 0x9E3779B1        # seed_hi and seed_lo both non-zero and different: swapped key words show
SEED_LO, SEED_HI = SEED & 0xFFFFFFFF, SEED >> 32
MAX_AMBIGUOUS = 0.02
ENV_TAG = 77


def _vec(v):
    return "[" + ", ".join(repr(float(x)) for x in v) + "]"


def _camera_yaml(W, H, look_from, look_at, up, fov, aperture, focus, background):
    return f"""film:
    width: {W}
    height: {H}
    samples: 1
    output: out.png
camera:
    position: {_vec(look_from)}
    look_at: {_vec(look_at)}
    up: {_vec(up)}
    fov: {fov}
    aperture: {aperture}
    focal_distance: {focus}
    background: {background}
"""


def f64_camera(case):
    return F.camera(case["look_from"], case["look_at"], case["up"], case["fov"], case["W"] / case["H"],
                    case.get("aperture", 0.0), case.get("focus", 1.0))


# ------------------------------------------------------------------ background only: which environment texel each pixel read
BG_CASES = {
    # odd film sizes, a map coarser than the film, non-square aspect
    "odd_257x129": dict(W=257, H=129, env=(64, 32), look_from=(0, 0, 0), look_at=(0.3, 0.2, 1.0), up=(0, 1, 0), fov=70),
    # the thinnest film the API takes (W-1 and H-1 are divided by) and a 1-texel-wide map
    "film_64x2_map_1x8": dict(W=64, H=2, env=(1, 8), look_from=(0, 0, 0), look_at=(1, 0.3, 0.5), up=(0, 1, 0), fov=100),
    # looking along -x: the seam phi = +-pi (column 0 against column W-1) runs down the middle of the film
    "seam_minus_x": dict(W=96, H=64, env=(200, 100), look_from=(0, 0, 0), look_at=(-1, 0.1, 0), up=(0, 1, 0), fov=90),
    # looking nearly straight up: the pole v = 0 and every column of row 0 in view
    "pole_up": dict(W=80, H=80, env=(64, 32), look_from=(0, 0, 0), look_at=(1e-3, 1, 2e-3), up=(0, 0, 1), fov=60),
    "thin_lens": dict(W=64, H=48, env=(128, 64), look_from=(0.5, 0.2, -0.3), look_at=(0.5, 0.2, 1), up=(0, 1, 0), fov=55,
                      aperture=0.6, focus=2.0, thin=True),
}


def background_scene(tmp_path, case):
    """Equirect PNG whose texel (i, j) holds the bytes (i, j, ENV_TAG); one sphere behind the camera, nothing else."""
    from hobbyraytracer_amd import api
    EW, EH = case["env"]
    img = np.zeros((EH, EW, 3), np.uint8)
    img[..., 0] = np.arange(EW)[None, :]
    img[..., 1] = np.arange(EH)[:, None]
    img[..., 2] = ENV_TAG
    d = str(tmp_path)
    api.write_image(os.path.join(d, "env.png"), img)
    fwd = np.asarray(case["look_at"], float) - np.asarray(case["look_from"], float)
    behind = np.asarray(case["look_from"], float) - 50 * fwd / np.linalg.norm(fwd)
    y = _camera_yaml(case["W"], case["H"], case["look_from"], case["look_at"], case["up"], case["fov"], case.get("aperture", 0.0),
                     case.get("focus", 1.0), "sky")
    y += f"""textures:
  - name: sky
    type: environment
    path: env.png
materials:
  - name: grey
    type: lambertian
    albedo: [0.5, 0.5, 0.5]
objects:
  - type: sphere
    center: {_vec(behind)}
    radius: 1.0
    material: grey
"""
    p = os.path.join(d, "bg.yaml")
    with open(p, "w") as f:
        f.write(y)
    return api.HostScene(p, d)


_LDR = (np.arange(256) / 255.0) ** 2.2      # stbi_loadf's ldr_to_hdr of a PNG byte


def decode_env(film):
    """Film values (linear, one sample) -> the PNG bytes they came from; the decode residual must be far below the spacing."""
    k = np.abs(film[..., None].astype(np.float64) - _LDR).argmin(-1)
    assert np.all(np.abs(film - _LDR[k]) <= 1e-5 * np.maximum(_LDR[k], 1e-6)), "a film value is no environment texel"
    return k


def check_background(film, case, rect, sample, seed_lo=SEED_LO, seed_hi=SEED_HI, rows=None):
    """film: (h, w, 3) for global columns rect.x0.. and global rows `rows` (default rect.y0..).  -> ambiguous fraction."""
    x0, y0, w, h = rect
    rows = np.arange(y0, y0 + h) if rows is None else np.asarray(rows)
    py, px = np.meshgrid(rows, np.arange(x0, x0 + w), indexing="ij")
    EW, EH = case["env"]
    _, d = F.primary_rays(f64_camera(case), case["W"], case["H"], px, py, sample, seed_lo, seed_hi, case.get("thin", False))
    u, v = F.miss_uv(d)
    du, dv = F.miss_uv_delta(d)
    i, ilo, ihi, ai = F.band_wrap(lambda x: F.env_index(x, EW), u, du)
    j, jlo, jhi, aj = F.band(lambda x: F.env_index(x, EH), v, dv)
    k = decode_env(film)
    gi, gj, tag = k[..., 0], k[..., 1], k[..., 2]
    assert np.all(tag == ENV_TAG), "channel order"
    amb = ai | aj
    frac = float(amb.mean())
    assert frac < MAX_AMBIGUOUS, f"ambiguity band too wide: {frac:.4f}"
    bad = ~amb & ((gi != i) | (gj != j))
    assert not bad.any(), _first_bad(bad, px, py, gi, gj, i, j)
    ok_band = ((gi == ilo) | (gi == ihi)) & ((gj == jlo) | (gj == jhi))
    assert np.all(ok_band[amb]), "a pixel in the band read a texel that is no neighbour of the float64 one"
    return frac


def _first_bad(bad, px, py, gi, gj, i, j):
    n = int(bad.sum())
    a = tuple(x[0] for x in np.nonzero(bad))
    return (f"{n} pixels read another texel than the float64 reference, first: pixel ({px[a]}, {py[a]}) got ({gi[a]}, {gj[a]}) "
            f"expected ({i[a]}, {j[a]})")


# ------------------------------------------------------------------ emitters: image texture, checkered texture
EMIT_W, EMIT_H = 72, 56
EMIT_CAM = dict(W=EMIT_W, H=EMIT_H, look_from=(0.1, 0.05, 0.0), look_at=(0.1, 0.05, -1.0), up=(0, 1, 0), fov=75)
RECT = dict(x=(-1.5, 1.7), y=(-0.9, 1.1), k=-2.0)                 # xy_rect: its four edges are in view
SPHERE = dict(center=(-2.6, 0.2, -0.4), radius=1.3)               # seen from +x: the seam of sphere.cpp's u (z = 0, x < 0) in view
SPHERE_CAM = dict(W=64, H=64, look_from=(0.0, 0.0, 0.0), look_at=(-1.0, 0.1, -0.1), up=(0, 1, 0), fov=80)
IMAGE_SIZES = [(37, 23), (1, 1), (1, 19)]


def _emitter_scene(tmp_path, cam, obj_yaml, albedo, textures_yaml, background="[0, 0, 0]", name="emit"):
    from hobbyraytracer_amd import api
    d = str(tmp_path)
    y = _camera_yaml(cam["W"], cam["H"], cam["look_from"], cam["look_at"], cam["up"], cam["fov"], 0.0, 1.0, background)
    y += textures_yaml + f"""materials:
  - name: lamp
    type: diffuse_light
    albedo: {albedo}
    strength: 2
objects:
{obj_yaml}"""
    p = os.path.join(d, f"{name}.yaml")
    with open(p, "w") as f:
        f.write(y)
    return api.HostScene(p, d)


def _rect_yaml():
    return f"""  - type: xy_rect
    x: {_vec(RECT['x'])}
    y: {_vec(RECT['y'])}
    k: {RECT['k']}
    material: lamp
"""


def _sphere_yaml(s):
    return f"""  - type: sphere
    center: {_vec(s['center'])}
    radius: {s['radius']}
    material: lamp
"""


def image_scene(tmp_path, size, shape):
    """DiffuseLight (strength 2) with an image albedo whose texel (i, j) holds (i + 1, j + 1, 200); shape 'rect' or 'sphere'."""
    from hobbyraytracer_amd import api
    TW, TH = size
    img = np.zeros((TH, TW, 3), np.uint8)
    img[..., 0] = 1 + np.arange(TW)[None, :]
    img[..., 1] = 1 + np.arange(TH)[:, None]
    img[..., 2] = 200
    api.write_image(os.path.join(str(tmp_path), "tex.png"), img)
    tex = "textures:\n  - name: tex\n    type: image\n    path: tex.png\n"
    if shape == "rect":
        return _emitter_scene(tmp_path, EMIT_CAM, _rect_yaml(), "tex", tex, name="img_rect")
    return _emitter_scene(tmp_path, SPHERE_CAM, _sphere_yaml(SPHERE), "tex", tex, name="img_sphere")


def _rect_prediction(o, d):
    t, p, _ = F.rect_hit(o, d, 2, *RECT["x"], *RECT["y"], RECT["k"])
    u, v = F.rect_uv(p, 0, 1, *RECT["x"], *RECT["y"])
    scale = np.linalg.norm(o, axis=-1) + np.linalg.norm(p, axis=-1)
    front = np.isfinite(t) & (t > 0)
    return u, v, F.EPS * scale / (RECT["x"][1] - RECT["x"][0]), F.EPS * scale / (RECT["y"][1] - RECT["y"][0]), front, p, scale


def _sphere_prediction(o, d):
    c, r = np.asarray(SPHERE["center"], float), SPHERE["radius"]
    t0, _, dist = F.sphere_roots(o, d, c, r)
    p = o + t0[..., None] * d
    n = (p - c) / r
    u, v = F.sphere_uv(n)
    scale = np.linalg.norm(o, axis=-1) + np.linalg.norm(p, axis=-1) + np.linalg.norm(c)
    rxz = np.maximum(np.hypot(n[..., 0], n[..., 2]), 1e-300)
    dn = F.EPS * scale / r
    hit = np.isfinite(t0) & (t0 > 0)
    sil = np.abs(dist - r) < F.EPS * scale             # silhouette: fp32 may hit or miss
    return u, v, dn / (2 * np.pi * rxz), dn / (np.pi * rxz), hit, sil, p, scale


def _pixels(cam):
    py, px = np.meshgrid(np.arange(cam["H"]), np.arange(cam["W"]), indexing="ij")
    o, d = F.primary_rays(f64_camera(cam), cam["W"], cam["H"], px, py, 0, SEED_LO, SEED_HI)
    return o, d


def check_image(film, size, shape):
    """Every pixel: 2 * texel / 255 of the float64 texel, or the black background on a miss.  -> ambiguous fraction."""
    TW, TH = size
    cam = EMIT_CAM if shape == "rect" else SPHERE_CAM
    o, d = _pixels(cam)
    if shape == "rect":
        u, v, du, dv, front, _, _ = _rect_prediction(o, d)
        fi = lambda x: np.where(front & (x >= 0) & (x <= 1), F.image_i(x, TW), -1)        # noqa: E731  -1: off the rect
        fj = lambda x: np.where(front & (x >= 0) & (x <= 1), F.image_j(x, TH), -1)        # noqa: E731
        i, ilo, ihi, ai = F.band(fi, u, du)
        j, jlo, jhi, aj = F.band(fj, v, dv)
        sil = np.zeros(u.shape, bool)
    else:
        u, v, du, dv, hit, sil, _, _ = _sphere_prediction(o, d)
        i, ilo, ihi, ai = F.band_wrap(lambda x: np.where(hit, F.image_i(x, TW), -1), u, du)
        j, jlo, jhi, aj = F.band(lambda x: np.where(hit, F.image_j(x, TH), -1), v, dv)
    miss = (i < 0) | (j < 0)
    i, j = np.where(miss, -1, i), np.where(miss, -1, j)
    b = np.rint(film.astype(np.float64) * 255.0 / 2.0).astype(np.int64)
    assert np.allclose(film, b * np.float32(2.0 / 255.0), rtol=1e-6, atol=0), "a film value is no 2 * texel / 255"
    gi, gj = b[..., 0] - 1, b[..., 1] - 1
    gmiss = (b == 0).all(-1)
    assert np.all((b[..., 2] == 200) | gmiss), "channel order"
    gi, gj = np.where(gmiss, -1, gi), np.where(gmiss, -1, gj)
    amb = ai | aj | sil
    frac = float(amb.mean())
    assert frac < MAX_AMBIGUOUS, f"ambiguity band too wide: {frac:.4f}"
    assert (~miss).mean() > 0.3, "the emitter must fill a good part of the view"
    py, px = np.meshgrid(np.arange(cam["H"]), np.arange(cam["W"]), indexing="ij")
    bad = ~amb & ((gi != i) | (gj != j))
    assert not bad.any(), _first_bad(bad, px, py, gi, gj, i, j)
    ok = (gmiss & (sil | (ilo < 0) | (ihi < 0) | (jlo < 0) | (jhi < 0))) | \
         (((gi == ilo) | (gi == ihi)) & ((gj == jlo) | (gj == jhi)))
    assert np.all(ok[amb]), "a pixel in the band read a texel that is no neighbour of the float64 one"
    return frac


# CheckeredTexture: k = 0.13 on the xz_rect (sin(10 * 0.13) = 0.96).  A k at a multiple of pi / 10 would make sin(10 p.y) a
# rounding residue of either sign that no reference can predict.  The background is the same checker: the miss branch looks it
# up at p = (0, 0, 0), where sines == 0 must give the EVEN colour (texture.cpp:20: only sines < 0 is odd).
CHECK_EVEN, CHECK_ODD = (1.0, 0.5, 0.25), (0.25, 0.5, 1.0)
CHECK_RECT = dict(x=(-3.0, 3.0), z=(-4.0, -0.5), k=0.13)
CHECK_CAM = dict(W=64, H=48, look_from=(0.05, 1.0, 0.5), look_at=(0.0, 0.0, -2.0), up=(0, 1, 0), fov=70)
CHECK_SPHERE = dict(center=(0.4, 0.3, -3.0), radius=1.0)
CHECK_SPHERE_CAM = dict(W=64, H=64, look_from=(0.0, 0.2, 0.0), look_at=(0.4, 0.3, -3.0), up=(0, 1, 0), fov=45)


def checker_scene(tmp_path, shape):
    tex = f"""textures:
  - name: chk
    type: checkered
    even: {_vec(CHECK_EVEN)}
    odd: {_vec(CHECK_ODD)}
"""
    if shape == "rect":
        r = CHECK_RECT
        obj = f"""  - type: xz_rect
    x: {_vec(r['x'])}
    z: {_vec(r['z'])}
    k: {r['k']}
    material: lamp
"""
        return _emitter_scene(tmp_path, CHECK_CAM, obj, "chk", tex, background="chk", name="chk_rect")
    return _emitter_scene(tmp_path, CHECK_SPHERE_CAM, _sphere_yaml(CHECK_SPHERE), "chk", tex, background="chk", name="chk_sphere")


def check_checker(film, shape):
    """Hit: 2 * (even | odd) by the float64 sign of the sines; miss: the checker at p = 0, i.e. even.  -> ambiguous fraction."""
    cam = CHECK_CAM if shape == "rect" else CHECK_SPHERE_CAM
    o, d = _pixels(cam)
    if shape == "rect":
        r = CHECK_RECT
        t, p, hit = F.rect_hit(o, d, 1, *r["x"], *r["z"], r["k"])
        scale = np.linalg.norm(o, axis=-1) + np.linalg.norm(p, axis=-1)
        ex = F.EPS * scale
        sil = hit & ((np.abs(p[..., 0] - np.asarray(r["x"])[:, None, None]).min(0) < ex) |
                     (np.abs(p[..., 2] - np.asarray(r["z"])[:, None, None]).min(0) < ex))
        sil |= ~hit & np.isfinite(t) & (t > 0) & (((p[..., 0] > r["x"][0] - ex) & (p[..., 0] < r["x"][1] + ex)) &
                                                   ((p[..., 2] > r["z"][0] - ex) & (p[..., 2] < r["z"][1] + ex)))
    else:
        c, rad = np.asarray(CHECK_SPHERE["center"]), CHECK_SPHERE["radius"]
        t0, _, dist = F.sphere_roots(o, d, c, rad)
        hit = np.isfinite(t0) & (t0 > 0)
        p = o + t0[..., None] * d
        scale = np.linalg.norm(o, axis=-1) + np.linalg.norm(p, axis=-1) + np.linalg.norm(c)
        sil = np.abs(dist - rad) < F.EPS * scale
    odd = F.checker_odd(np.where(hit[..., None], p, 0.0))
    amb = sil | (hit & F.checker_ambiguous(np.where(hit[..., None], p, 1.0), scale))
    frac = float(amb.mean())
    assert frac < MAX_AMBIGUOUS, f"ambiguity band too wide: {frac:.4f}"
    assert hit.mean() > 0.3 and (~hit).mean() > 0.05, "the view must hold both the emitter and the background"
    classes = {0: np.array(CHECK_EVEN) * 2, 1: np.array(CHECK_ODD) * 2, 2: np.array(CHECK_EVEN), 3: np.array(CHECK_ODD)}
    got = np.full(film.shape[:2], -1)
    for k, c in classes.items():
        got[np.abs(film - c.astype(np.float32)).max(-1) <= 1e-6] = k
    assert np.all(got >= 0), "a film value is none of the four checker colours"
    want = np.where(hit, odd.astype(int), 2)             # a miss: the checker at p = 0 -> even
    bad = ~amb & (got != want)
    assert not bad.any(), f"{int(bad.sum())} pixels differ from the float64 checker (got {got[bad][:8]}, want {want[bad][:8]})"
    assert (want == 0).any() and (want == 1).any() and (want == 2).any(), "both checker colours and the background in view"
    return frac


# ------------------------------------------------------------------ ConstantMedium free path through closest_hit
MEDIUM_BOX = ((-1.0, -0.5, -0.8), (1.2, 0.7, 0.9))
MEDIUM_SPHERE = ((0.3, -0.2, 0.1), 1.1)
MEDIUM_N = 20000                      # rays per ray set; five sets per medium
PIXEL0 = 3000                         # closest_hit keys ray i as (PIXEL0 + i, sample 0, bounce 0)
KS_CRIT = 1.95                        # Kolmogorov-Smirnov: D * sqrt(n) < 1.95 (p ~ 0.001)
U0_PIXEL = 14654730                   # first pixel with word x of (pixel, 0, 0, RNG_MEDIUM | 0 << 8) < 256 under SEED: u = 0


def medium_scene(tmp_path, kind, density, geom=None, name="medium"):
    from hobbyraytracer_amd import api
    if kind == "box":
        lo, hi = geom or MEDIUM_BOX
        b = f"        type: box\n        min: {_vec(lo)}\n        max: {_vec(hi)}\n"
    else:
        c, r = geom or MEDIUM_SPHERE
        b = f"        type: sphere\n        center: {_vec(c)}\n        radius: {r}\n"
    y = _camera_yaml(8, 8, (0, 0, 9), (0, 0, 0), (0, 1, 0), 40, 0.0, 1.0, "[0, 0, 0]")
    y += f"""materials:
  - name: unused
    type: lambertian
    albedo: [0.5, 0.5, 0.5]
objects:
  - type: constant_medium
    density: {density}
    colour: [0.9, 0.4, 0.4]
    boundary:
{b}"""
    p = os.path.join(str(tmp_path), f"{name}.yaml")
    with open(p, "w") as f:
        f.write(y)
    return api.HostScene(p, str(tmp_path))


def _geom(kind):
    return MEDIUM_BOX if kind == "box" else MEDIUM_SPHERE


def _centre_extent(kind):
    if kind == "box":
        lo, hi = (np.asarray(a) for a in MEDIUM_BOX)
        return (lo + hi) / 2, (hi - lo) / 2
    c, r = MEDIUM_SPHERE
    return np.asarray(c), np.full(3, r)


def medium_ray_sets(kind, seed=11):
    """{name: (origins, directions, t_min, t_max)}; every direction has a length in [0.3, 3] (not normalised)."""
    r = np.random.default_rng(seed)
    n = MEDIUM_N
    c, ext = _centre_extent(kind)
    lens = r.uniform(0.3, 3.0, (n, 1))

    def unit(k):
        v = r.normal(size=(k, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def outside():
        o = c + 4.0 * unit(n)
        tgt = c + r.uniform(-1.3, 1.3, (n, 3)) * ext     # some aim past the boundary: misses
        return o, (tgt - o) / np.linalg.norm(tgt - o, axis=1, keepdims=True) * lens

    inside_o = c + r.uniform(-0.9, 0.9, (n, 3)) * ext
    if kind == "sphere":
        inside_o = c + unit(n) * (ext[0] * r.uniform(0, 0.9, (n, 1)) ** (1 / 3))
    sets = {}
    o, d = outside()
    sets["outside"] = (o, d, 0.001, float("inf"))
    sets["inside_tmin"] = (inside_o, unit(n) * lens, 0.001, float("inf"))             # t1 < 0 clamps to t_min
    sets["inside_behind"] = (inside_o, unit(n) * lens, -50.0, float("inf"))           # t1 < 0 kept, then clamps to 0
    o, d = outside()
    sets["short_tmax"] = (o, d, 0.001, 4.0 / lens[:, 0].mean())                      # t_max cuts most chords
    # grazing: lines that pass the sphere at r (1 +- 1e-2), or the box through points next to its edges
    o = c + 4.0 * unit(n)
    if kind == "sphere":
        radial = o - c
        side = np.cross(radial, unit(n))
        side /= np.linalg.norm(side, axis=1, keepdims=True)
        tgt = c + side * ext[0] * (1 + r.uniform(-1e-2, 1e-2, (n, 1)))
    else:
        tgt = c + ext * np.sign(r.normal(size=(n, 3))) * (1 + r.uniform(-1e-2, 1e-2, (n, 3)))
        keep = r.integers(0, 3, n)                        # one coordinate anywhere on the face: lines past an edge
        tgt[np.arange(n), keep] = c[keep] + r.uniform(-1, 1, n) * ext[keep]
    sets["grazing"] = (o, (tgt - o) / np.linalg.norm(tgt - o, axis=1, keepdims=True) * lens, 0.001, float("inf"))
    return {k: (np.asarray(a, np.float32), np.asarray(b, np.float32), t0, t1) for k, (a, b, t0, t1) in sets.items()}


def medium_u(n, pixel0=PIXEL0, seed_lo=SEED_LO, seed_hi=SEED_HI, prim=0):
    x = F.draw(seed_lo, seed_hi, np.arange(pixel0, pixel0 + n, dtype=np.uint64), 0, 0, F.RNG_MEDIUM, prim)[0]
    return F.u01(x)


def check_medium(hits, kind, density, o, d, t_min, t_max, u, geom=None):
    """prim, t and p against float64 outside the hit-or-miss band.  -> (ambiguous fraction, t1 after the clamps, ambiguous mask)."""
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    g = geom or _geom(kind)
    t_ref, t1, amb = F.medium_free_path(kind, g, np.float64(np.float32(density)), o64, d64, t_min, t_max, u)
    assert not np.isnan(hits["t"]).any() and not np.isnan(hits["p"]).any(), "NaN in a hit record"
    frac = float(amb.mean())
    assert frac < MAX_AMBIGUOUS, f"ambiguity band too wide: {frac:.4f}"
    want = np.isfinite(t_ref)
    got = hits["prim"] >= 0
    assert np.all(hits["prim"][got] == 0)
    bad = ~amb & (got != want)
    assert not bad.any(), f"{int(bad.sum())} rays: hit/miss differs from float64 (first {np.nonzero(bad)[0][:5]})"
    both = ~amb & got
    L = np.linalg.norm(d64, axis=1)
    # rtol 1e-5 on t; the absolute term is the fp32 resolution of the boundary's t: 64 ulps of (|o| + extent) / |d|, and for a
    # sphere the error bound of its roots
    atol = F.EPS * (np.linalg.norm(o64, axis=1) + F._extent(g)) / L
    if kind == "sphere":                  # plus the conditioning of the sphere's roots near a tangent
        atol = atol + F.sphere_root_error(o64, d64, *g)
    err = np.abs(hits["t"][both] - t_ref[both])
    assert np.all(err <= 1e-5 * np.abs(t_ref[both]) + atol[both]), f"t: worst {np.max(err / (np.abs(t_ref[both]) + atol[both]))}"
    p_ref = o64 + t_ref[:, None] * d64
    perr = np.abs(hits["p"][both] - p_ref[both]).max(1)
    pscale = np.linalg.norm(o64, axis=1) + np.abs(t_ref)[:] * L
    # p inherits t's tolerance along d, plus 64 ulps of its own magnitude
    assert np.all(perr <= ((1e-5 * np.abs(t_ref) + atol) * L + F.EPS * pscale)[both]), "hit point p = o + t d"
    return frac, t1, amb


def ks_free_path(hits, kind, density, o, d, amb):
    """(t - t1) |d| of the hits of an unclipped ray set (origins outside, t_max = inf) against Exp(rho) truncated at the chord:
    F(x) = (1 - exp(-rho x)) / (1 - exp(-rho chord)) must be uniform (Kolmogorov-Smirnov, D sqrt(n) < KS_CRIT), and the number
    of hits must be sum(1 - exp(-rho chord)) within 5 sigma.  Independent of the RNG restatement.  -> (D, n)."""
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    t1, t2, ok, _ = F.medium_boundary(kind, _geom(kind), o64, d64)
    L = np.linalg.norm(d64, axis=1)
    rho = float(np.float32(density))
    sel = ok & ~amb & (t1 > 0.001)
    chord = (t2[sel] - t1[sel]) * L[sel]
    p_hit = -np.expm1(-rho * chord)
    got = hits["prim"][sel] >= 0
    n_exp, sd = p_hit.sum(), np.sqrt((p_hit * (1 - p_hit)).sum())
    assert abs(got.sum() - n_exp) < 5 * sd, f"hits {got.sum()} vs expected {n_exp:.1f} +- {sd:.1f}"
    x = (hits["t"][sel][got].astype(np.float64) - t1[sel][got]) * L[sel][got]
    cdf = np.sort(np.clip(-np.expm1(-rho * x) / p_hit[got], 0, 1))
    n = len(cdf)
    k = np.arange(1, n + 1)
    D = max((k / n - cdf).max(), (cdf - (k - 1) / n).max())
    assert n > 1000 and D * np.sqrt(n) < KS_CRIT, f"KS D = {D:.4f}, n = {n}"
    return D, n


THIN_BOX = ((0.0, -1.0, -1.0), (5e-5, 1.0, 1.0))      # thinner than the 1e-4 re-entry step along x
SLAB_BOX = ((0.0, -1.0, -1.0), (2e-4, 1.0, 1.0))      # thicker than it
THIN_DENSITY = 2e4                                    # a 5e-5 chord would be hit 63 % of the time, a 2e-4 one 98 %


def check_thin_and_u0(make_world, tmp_path, params):
    """constantMedium.cpp:14: rec2 is searched from rec1.t + 0.0001, so a boundary thinner than that along the ray is no hit;
    and the ray keyed by U0_PIXEL draws u = 0 (ln 0 = -inf): it misses, and nothing is NaN."""
    r = np.random.default_rng(5)
    n = 4000
    o = np.stack([np.full(n, -1.0), r.uniform(-0.5, 0.5, n), r.uniform(-0.5, 0.5, n)], 1)
    d = np.stack([np.ones(n), r.uniform(-0.2, 0.2, n), r.uniform(-0.2, 0.2, n)], 1) * r.uniform(0.6, 1.5, (n, 1))        # |d.x| <= 1.5: the slab's chord stays above 1e-4 in t
    o, d = o.astype(np.float32), d.astype(np.float32)
    u = medium_u(n)
    hit_counts = []
    for geom, name in ((THIN_BOX, "thin"), (SLAB_BOX, "slab")):
        hs = medium_scene(tmp_path, "box", THIN_DENSITY, geom, name=name)
        hits = make_world(hs).closest_hit(params, o, d, 0.001, float("inf"), PIXEL0)
        check_medium(hits, "box", THIN_DENSITY, o, d, 0.001, float("inf"), u, geom=geom)
        hit_counts.append(int((hits["prim"] >= 0).sum()))
    assert hit_counts[0] == 0, "a boundary 5e-5 thick along the ray must give no hit"
    assert hit_counts[1] > 0.9 * n, "a boundary 2e-4 thick along the ray is entered and left"
    # u = 0
    for kind in ("box", "sphere"):
        hs = medium_scene(tmp_path, kind, 3.0, name=f"u0_{kind}")
        c, _ = _centre_extent(kind)
        o1 = np.array([c + [0.0, 0.0, 5.0]], np.float32)
        d1 = np.array([[0.0, 0.0, -1.0]], np.float32)
        h = make_world(hs).closest_hit(params, o1, d1, 0.001, float("inf"), U0_PIXEL)
        assert h["prim"][0] == -1, "u = 0: hit_distance = +inf, no hit"
        assert np.isfinite(h["t"]).all() and np.isfinite(h["p"]).all()
        # the neighbouring counter (u > 0) does hit the medium along the same ray: the miss above is u's doing
        h2 = make_world(hs).closest_hit(params, o1, d1, 0.001, float("inf"), U0_PIXEL + 1)
        u2 = float(medium_u(1, U0_PIXEL + 1)[0])
        chord = MEDIUM_BOX[1][2] - MEDIUM_BOX[0][2] if kind == "box" else 2 * MEDIUM_SPHERE[1]   # the ray runs through the centre
        assert (h2["prim"][0] == 0) == (-np.log(u2) / np.float32(3.0) <= chord)
