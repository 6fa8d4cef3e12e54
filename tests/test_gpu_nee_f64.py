"""Float64 pin of next-event estimation (HRT_FLAG_NEE): a Lambertian xz_rect floor under an xz_rect light, black
background, 1 spp, max_depth 2.  Every pixel is restated in numpy float64 from tests/f64_reference.py's Philox, primary_rays and
rect_hit and the definitions of DESIGN.md 4.5 alone: the camera ray meets the floor; the floor vertex (bounce 0) scatters with the
RNG_SCATTER draw of (pixel, 0, 0) and, through its RNG_LIGHT draw of (pixel, 0, 0), samples the light -- words y and z the point,
p_l = dist^2 / (A |cos|), p_b = cos / pi -- and adds albedo Le p_b q / (p_b^2 + q^2); the bounce adds albedo Le p_b^2 / (p_b^2 + q^2)
when it hits the light.  So the RNG layout of the light sample and the MIS arithmetic are pinned per sample, not only in distribution.
A bounce that meets the light within the ambiguity band of its edge may take either value; the band holds < 2 % of the samples."""
import os

import numpy as np
import pytest

from tests import f64_reference as F

pytestmark = pytest.mark.gpu

RNG_LIGHT = 6                  # hrt_rng.h
SEED = 0x0000123456789ABC
W, H = 64, 48
ALBEDO, LE = 0.5, np.array([0.9, 0.8, 0.7])
HALF, K_LIGHT, T_MIN = 0.5, 1.0, 0.001
CAM = dict(look_from=(0.15, 0.7, 0.1), look_at=(0.15, 0.0, 0.1001), up=(0.0, 0.0, -1.0), fov=70.0)

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
    albedo: [{LE[0]}, {LE[1]}, {LE[2]}]
    strength: 1
objects:
  - type: xz_rect
    x: [-50, 50]
    z: [-50, 50]
    k: 0
    material: floor
  - type: xz_rect
    x: [{-HALF}, {HALF}]
    z: [{-HALF}, {HALF}]
    k: {K_LIGHT}
    material: lamp
"""


def restate(seed_lo, seed_hi):
    """-> (NEE film, default film, ambiguous mask), float64, [H, W, 3] / [H, W]"""
    cam = F.camera(CAM["look_from"], CAM["look_at"], CAM["up"], CAM["fov"], W / H)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pix = (py * W + px).astype(np.uint64)
    o, d = F.primary_rays(cam, W, H, px, py, 0, seed_lo, seed_hi)
    t, p, hit = F.rect_hit(o, d, 1, -50.0, 50.0, -50.0, 50.0, 0.0)
    assert hit.all() and (t > T_MIN).all()
    n = np.array([0.0, 1.0, 0.0])
    area = (2 * HALF) ** 2
    # the bounce: sd = n + sphericalRand(1) of the RNG_SCATTER draw (hrt_rng.h spherical_rand), bounce 0
    u = F.draw(seed_lo, seed_hi, pix, 0, 0, F.RNG_SCATTER)
    theta = F.u01(u[0]) * (2 * np.pi)
    z = F.u01(u[1]) * 2.0 - 1.0
    sp = np.sqrt(1.0 - z * z)
    sd = n + np.stack([sp * np.cos(theta), sp * np.sin(theta), z], axis=-1)
    tl, yl, hitl = F.rect_hit(p, sd, 1, -HALF, HALF, -HALF, HALF, K_LIGHT)
    hitl &= tl >= T_MIN
    wl = sd / np.linalg.norm(sd, axis=-1, keepdims=True)
    pb_b = np.maximum(wl[..., 1], 0.0) / np.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        q_b = ((yl - p) ** 2).sum(-1) / (area * np.abs(wl[..., 1]))
        w_b = np.where(hitl, pb_b ** 2 / (pb_b ** 2 + q_b ** 2), 0.0)
    # the light sample: RNG_LIGHT draw of (pixel, sample 0, bounce 0); words y / z = the point, P_sel = 1
    v = F.draw(seed_lo, seed_hi, pix, 0, 0, RNG_LIGHT)
    y = np.stack([-HALF + F.u01(v[1]) * (2 * HALF), np.full(px.shape, K_LIGHT), -HALF + F.u01(v[2]) * (2 * HALF)], axis=-1)
    dl = y - p
    dist2 = (dl ** 2).sum(-1)
    w = dl / np.sqrt(dist2)[..., None]
    pb = w[..., 1] / np.pi
    q = dist2 / (area * np.abs(w[..., 1]))
    g = pb * q / (pb * pb + q * q)
    nee = (ALBEDO * (w_b + g))[..., None] * LE
    default = (ALBEDO * hitl)[..., None] * LE
    # ambiguity band of the bounce's hit-or-miss at the light's edges
    delta = F.EPS * (1.0 + np.abs(yl[..., [0, 2]]).max(-1) + np.linalg.norm(yl - p, axis=-1))
    with np.errstate(invalid="ignore"):
        edge = np.minimum(np.abs(np.abs(yl[..., 0]) - HALF), np.abs(np.abs(yl[..., 2]) - HALF))
        amb = np.isfinite(tl) & (tl > 0) & (np.abs(yl[..., [0, 2]]).max(-1) < HALF + delta) & (edge < delta)
    return nee, default, amb, (ALBEDO * g)[..., None] * LE


def test_nee_film_equals_the_float64_restatement(built, tmp_path):
    from hobbyraytracer_amd import api
    path = os.path.join(str(tmp_path), "floor.yaml")
    with open(path, "w") as f:
        f.write(YAML)
    hs = api.HostScene(path, str(tmp_path))
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        cam = hs.camera(W, H)
        nee_got, st = dev.render_tile(cam, api.default_params(W, H, 1, max_depth=2, seed=SEED, nee=True))
        def_got, st0 = dev.render_tile(cam, api.default_params(W, H, 1, max_depth=2, seed=SEED))
    finally:
        dev.close()
    assert st.shadow_rays == W * H and st.rays == st0.rays == 2 * W * H
    nee, default, amb, direct_only = restate(SEED & 0xFFFFFFFF, SEED >> 32)
    print(f"ambiguous fraction {amb.mean():.5f}, bounce hits {int((default[..., 0] > 0).sum())} of {W * H}")
    assert amb.mean() < 0.02
    assert (default[..., 0] > 0).sum() > 20          # the bounce term is exercised, not only the light sample
    tol = 2e-4 * np.abs(nee) + 1e-7
    ok = np.abs(nee_got - nee) <= tol
    # inside the band the bounce may have missed: the light sample's term alone
    ok |= amb[..., None] & (np.abs(nee_got - direct_only) <= 2e-4 * np.abs(direct_only) + 1e-7)
    bad = np.argwhere(~ok.all(-1))
    assert bad.size == 0, [(tuple(i), nee_got[tuple(i)], nee[tuple(i)]) for i in bad[:5]]
    okd = (np.abs(def_got - default) <= 2e-4 * np.abs(default) + 1e-7) | amb[..., None]
    assert okd.all()
