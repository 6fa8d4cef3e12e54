"""Float64 pin of next-event estimation over the emitter table (HRT_FLAG_NEE_EMITTERS): a Lambertian floor under a
wrapped emissive mesh triangle (tilted in the OBJ, under rotate_y, scale and translate) and an xz_rect light, black background, 1 spp,
max_depth 2.  Every pixel is restated in numpy float64 from tests/f64_reference.py's Philox and the definitions of DESIGN.md 4.7 alone,
with the table read back through hrt_emitter_table_build: the floor vertex (bounce 0) chooses a light by the alias table (slot from word
x of RNG_LIGHT aux 0, coin from word x of aux 1), samples a point (words y, z; the square-root parametrisation on the triangle),
p_l = dist^2 / (A |n.w|), p_b = cos / pi, and adds albedo Le p_b q / (p_b^2 + q^2) when the other light does not block it; the bounce
adds albedo Le p_b^2 / (p_b^2 + q^2) for the light it hits.  So the alias choice, the point, both densities and both MIS weights are
pinned per sample.  Samples within the ambiguity band of an edge (of the light the bounce meets, of the sampled triangle, or of the
other light's shadow) may take either value; the band holds < 2 % of the pixels."""
import os

import numpy as np
import pytest

from tests import f64_reference as F

pytestmark = pytest.mark.gpu

RNG_LIGHT = 6                  # hrt_rng.h
SEED = 0x0000123456789ABC
W, H = 64, 48
ALBEDO = 0.5
LE_RECT, LE_TRI = np.array([0.9, 0.8, 0.7]), np.array([0.4, 0.7, 1.0]) * 2.0
RECT = (-0.6, -0.1, -0.3, 0.3, 1.0)          # x0, x1, z0, z1, k
T_MIN = 0.001
CAM = dict(look_from=(0.15, 0.7, 0.1), look_at=(0.15, 0.0, 0.1001), up=(0.0, 0.0, -1.0), fov=70.0)
TRI_OBJ = "v -0.3 0 -0.25\nv 0.3 0.15 -0.25\nv 0 -0.1 0.35\nf 1 2 3\n"      # faces down; no quaternion: t keeps world units

YAML = f"""film:
    width: {W}
    height: {H}
    samples: 1
    output: out.png
camera:
    position: [{CAM['look_from'][0]}, {CAM['look_from'][1]}, {CAM['look_from'][2]}]
    look_at: [{CAM['look_at'][0]}, {CAM['look_at'][1]}, {CAM['look_at'][2]}]
    up: [0, 0, -1]
    fov: {CAM['fov']}
    aperture: 0
    focal_distance: 1
    background: [0, 0, 0]
materials:
  - name: floor
    type: lambertian
    albedo: [{ALBEDO}, {ALBEDO}, {ALBEDO}]
  - name: lamp
    type: diffuse_light
    albedo: [{LE_RECT[0]}, {LE_RECT[1]}, {LE_RECT[2]}]
    strength: 1
  - name: glow
    type: diffuse_light
    albedo: [{LE_TRI[0] / 2}, {LE_TRI[1] / 2}, {LE_TRI[2] / 2}]
    strength: 2
objects:
  - type: xz_rect
    x: [-50, 50]
    z: [-50, 50]
    k: 0
    material: floor
  - type: xz_rect
    x: [{RECT[0]}, {RECT[1]}]
    z: [{RECT[2]}, {RECT[3]}]
    k: {RECT[4]}
    material: lamp
  - type: mesh
    path: tri.obj
    material: glow
    transform:
        rotate_y: 30
        scale: [1.2, 1, 0.9]
        translate: [0.5, 1.1, 0.1]
"""


def _dot(a, b):
    return (a * b).sum(-1)


def tri_hit(o, d, v0, e1, e2):
    """(t, barycentric u, v) of the ray o + t d with the triangle v0 + u e1 + v e2 (Moeller-Trumbore, float64, no range tests)"""
    pv = np.cross(d, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / _dot(pv, e1)
        tv = o - v0
        u = _dot(tv, pv) * inv
        qv = np.cross(tv, e1)
        v = _dot(d, qv) * inv
        t = _dot(qv, e2) * inv
    return t, u, v


def rect_edge(p):
    x0, x1, z0, z1, _ = RECT
    return np.minimum(np.minimum(np.abs(p[..., 0] - x0), np.abs(p[..., 0] - x1)), np.minimum(np.abs(p[..., 2] - z0), np.abs(p[..., 2] - z1)))


def restate(tab, seed_lo, seed_hi):
    """-> (film [H, W, 3], bounce-ambiguous, sample-ambiguous, bounce term, sample term), float64"""
    cam = F.camera(CAM["look_from"], CAM["look_at"], CAM["up"], CAM["fov"], W / H)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pix = (py * W + px).astype(np.uint64)
    o, d = F.primary_rays(cam, W, H, px, py, 0, seed_lo, seed_hi)
    t, p, hit = F.rect_hit(o, d, 1, -50.0, 50.0, -50.0, 50.0, 0.0)
    assert hit.all() and (t > T_MIN).all()
    rec = tab["rec"].astype(np.float64)
    kinds = tab["kind"]
    assert list(kinds) == [16, 17] and list(tab["prim"]) == [1, 2]
    to, te1, te2 = rec[1, 4:7], rec[1, 8:11], rec[1, 12:15]
    ro, re1, re2 = rec[0, 4:7], rec[0, 8:11], rec[0, 12:15]
    A = rec[:, 7]
    nrm = [np.cross(re1, re2) / np.linalg.norm(np.cross(re1, re2)), np.cross(te1, te2) / np.linalg.norm(np.cross(te1, te2))]
    psel = tab["p_sel"].astype(np.float64)
    le = [LE_RECT, LE_TRI]
    delta = 64 * F.EPS * 4.0

    def q_of(e, x, y):
        dl = y - x
        d2 = _dot(dl, dl)
        w = dl / np.sqrt(d2)[..., None]
        return psel[e] * d2 / (A[e] * np.abs(_dot(w, nrm[e])))

    def hits(x, dd):
        """the rect's and the triangle's hits of x + t dd (t > T_MIN): (t_r, hit_r, y_r, edge_r), (t_t, hit_t, y_t, edge_t)"""
        tr, yr, hr = F.rect_hit(x, dd, 1, *RECT)
        hr &= tr > T_MIN
        tt, u, v = tri_hit(x, dd, to, te1, te2)
        ht = np.isfinite(tt) & (tt > T_MIN) & (u >= 0) & (v >= 0) & (u + v <= 1)
        yt = x + tt[..., None] * dd
        et = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(1 - u - v))
        return (tr, hr, yr, rect_edge(yr) / (1.0 + np.abs(yr).max(-1))), (tt, ht, yt, et)

    # the bounce: sd = n + sphericalRand(1) of the RNG_SCATTER draw, bounce 0
    n = np.array([0.0, 1.0, 0.0])
    u = F.draw(seed_lo, seed_hi, pix, 0, 0, F.RNG_SCATTER)
    theta = F.u01(u[0]) * (2 * np.pi)
    zz = F.u01(u[1]) * 2.0 - 1.0
    sp = np.sqrt(1.0 - zz * zz)
    sd = n + np.stack([sp * np.cos(theta), sp * np.sin(theta), zz], axis=-1)
    wl = sd / np.linalg.norm(sd, axis=-1, keepdims=True)
    pb_b = np.maximum(wl[..., 1], 0.0) / np.pi
    (tr, hr, yr, er), (tt, ht, yt, et) = hits(p, sd)
    first_r = hr & (~ht | (tr < tt))
    first_t = ht & ~first_r
    with np.errstate(divide="ignore", invalid="ignore"):
        q_b = np.where(first_r, q_of(0, p, yr), np.where(first_t, q_of(1, p, yt), 0.0))
        w_b = np.where(first_r | first_t, pb_b ** 2 / (pb_b ** 2 + q_b ** 2), 0.0)
    bounce = (ALBEDO * w_b)[..., None] * np.where(first_r[..., None], LE_RECT, np.where(first_t[..., None], LE_TRI, 0.0))
    amb_b = (np.isfinite(tr) & (tr > 0) & (er < delta)) | (np.isfinite(tt) & (tt > 0) & (et < delta))
    # the light sample: alias choice, point, densities
    v = F.draw(seed_lo, seed_hi, pix, 0, 0, RNG_LIGHT)
    coin = F.draw(seed_lo, seed_hi, pix, 0, 0, RNG_LIGHT, 1)[0]
    nE = len(psel)
    slot = ((v[0].astype(np.uint64) * np.uint64(nE)) >> np.uint64(32)).astype(np.int64)
    keep = F.u01(coin) < tab["thresh"].astype(np.float64)[slot]
    li = np.where(keep, slot, tab["alias"][slot])
    a, b = F.u01(v[1]), F.u01(v[2])
    s = np.sqrt(a)
    y = np.where((li == 0)[..., None], ro + a[..., None] * re1 + b[..., None] * re2,
                 to + (s * (1 - b))[..., None] * te1 + (s * b)[..., None] * te2)
    dl = y - p
    d2 = _dot(dl, dl)
    w = dl / np.sqrt(d2)[..., None]
    pb = np.maximum(w[..., 1], 0.0) / np.pi
    q = np.where(li == 0, q_of(0, p, y), q_of(1, p, y))
    g = pb * q / (pb * pb + q * q)
    # blocked by the other light before y (the shadow ray's hit must be the sampled one)
    (tr2, hr2, yr2, er2), (tt2, ht2, yt2, et2) = hits(p, dl)
    blocked = np.where(li == 0, ht2 & (tt2 < 1.0), hr2 & (tr2 < 1.0))
    amb_s = np.where(li == 0, np.isfinite(tt2) & (tt2 > 0) & (tt2 < 1.0) & (et2 < delta),
                     np.isfinite(tr2) & (tr2 > 0) & (tr2 < 1.0) & (er2 < delta))
    amb_s |= (li == 1) & (np.minimum(np.minimum(s * (1 - b), s * b), 1 - s) < delta)
    direct = np.where(blocked, 0.0, ALBEDO * g)[..., None] * np.where((li == 0)[..., None], LE_RECT, LE_TRI)
    return bounce + direct, amb_b, amb_s, bounce, direct, (li == 1).mean()


def test_emitter_film_equals_the_float64_restatement(built, tmp_path):
    from hobbyraytracer_amd import api
    (tmp_path / "tri.obj").write_text(TRI_OBJ)
    path = os.path.join(str(tmp_path), "floor.yaml")
    with open(path, "w") as f:
        f.write(YAML)
    hs = api.HostScene(path, str(tmp_path))
    tab = api.emitter_table_build(hs.flat_ptr)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        cam = hs.camera(W, H)
        got, st = dev.render_tile(cam, api.default_params(W, H, 1, max_depth=2, seed=SEED, nee_emitters=True))
        _, st0 = dev.render_tile(cam, api.default_params(W, H, 1, max_depth=2, seed=SEED))
    finally:
        dev.close()
    assert st.shadow_rays == W * H and st.rays == st0.rays == 2 * W * H
    film, amb_b, amb_s, bounce, direct, tri_share = restate(tab, SEED & 0xFFFFFFFF, SEED >> 32)
    amb = amb_b | amb_s
    print(f"ambiguous fraction {amb.mean():.5f}, bounce hits {int((bounce[..., 0] > 0).sum())}, triangle samples {tri_share:.3f}")
    assert amb.mean() < 0.02
    assert (bounce[..., 0] > 0).sum() > 20 and 0.1 < tri_share < 0.9     # both terms and both lights are exercised
    def close(ref):
        return np.abs(got - ref) <= 2e-4 * np.abs(ref) + 1e-7
    ok = close(film)
    # inside a band either term may be missing
    ok |= amb[..., None] & (close(direct) | close(bounce) | close(np.zeros_like(film)))
    bad = np.argwhere(~ok.all(-1))
    assert bad.size == 0, [(tuple(i), got[tuple(i)], film[tuple(i)]) for i in bad[:5]]
