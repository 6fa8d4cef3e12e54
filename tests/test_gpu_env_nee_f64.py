"""Float64 pin of environment-map sampling (HRT_FLAG_NEE_ENV): a Lambertian xz_rect floor under a map that is black but for
one block of texels of differing radiance, no table light, 1 spp, max_depth 2.  Every pixel is restated in numpy float64 from
tests/f64_reference.py's Philox, primary_rays and rect_hit, the cells of tests/env_tables.py and the definitions of DESIGN.md 4.6 alone:
the floor vertex (bounce 0) scatters with the RNG_SCATTER draw of (pixel, 0, 0); its environment sample takes the RNG_ENV draw of
(pixel, 0, 0) -- word x the row, y the column (the first CDF interval whose upper bound exceeds u01), z phi and w cos theta uniform in
the cell -- and adds albedo L pb pe / (pb^2 + pe^2) with pb = cos theta / pi and pe = P(cell) / solid angle of the cell the lookup
assigns to the direction; the bounce escapes and adds albedo L pb^2 / (pb^2 + pe^2).  The CDFs are the device's own (hrt_env_table_build,
pinned against float64 by tests/test_gpu_env_nee.py), so the row and column searches are restated exactly.  A direction within the
ambiguity band of a texel edge may read either texel; those pixels (< 2 %) are left out.  (The floor's normal has length 1, so the
second root of the shadow ray's length is 0 and the root choice, word x of the aux = 1 draw, has nothing to choose here.)"""
import os

import numpy as np
import pytest

from tests import env_tables as et
from tests import f64_reference as F

pytestmark = pytest.mark.gpu

RNG_ENV = 7                    # hrt_rng.h
SEED = 0x00000ABCDEF01234
W, H = 64, 48
MAP_W, MAP_H = 64, 32
BLOCK_I, BLOCK_J = (10, 20), (6, 12)
ALBEDO, T_MIN = 0.5, 0.001
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
    background: sky
textures:
  - name: sky
    type: environment
    path: block.hdr
materials:
  - name: floor
    type: lambertian
    albedo: [{ALBEDO}, {ALBEDO}, {ALBEDO}]
objects:
  - type: xz_rect
    x: [-50, 50]
    z: [-50, 50]
    k: 0
    material: floor
"""


def block_map():
    """grey texels of radiance 1 ... 3.5 in the block (so that pe differs from texel to texel), black elsewhere"""
    tex = np.zeros((MAP_H, MAP_W, 3), np.float32)
    for j in range(BLOCK_J[0], BLOCK_J[1] + 1):
        for i in range(BLOCK_I[0], BLOCK_I[1] + 1):
            tex[j, i] = 1.0 + 0.25 * (i % 5) + 0.5 * (j % 3)
    return tex


def lookup(d):
    """the texel background_value reads for direction d, float64, and whether d lies in the ambiguity band of a texel edge"""
    u, v = F.miss_uv(d)
    du, dv = F.miss_uv_delta(d)
    i, _, _, amb_i = F.band(lambda x: F.env_index(x, MAP_W), u, du)
    j, _, _, amb_j = F.band(lambda x: F.env_index(x, MAP_H), v, dv)
    return i, j, amb_i | amb_j


def restate(tex, marg, cond, seed_lo, seed_hi):
    """-> (--nee-env film, default film, ambiguous mask), float64, [H, W] (grey: one channel)"""
    cam = F.camera(CAM["look_from"], CAM["look_at"], CAM["up"], CAM["fov"], W / H)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pix = (py * W + px).astype(np.uint64)
    o, d = F.primary_rays(cam, W, H, px, py, 0, seed_lo, seed_hi)
    t, p, hit = F.rect_hit(o, d, 1, -50.0, 50.0, -50.0, 50.0, 0.0)
    assert hit.all() and (t > T_MIN).all()
    n = np.array([0.0, 1.0, 0.0])
    L = tex[..., 0].astype(np.float64)
    P = et.cell_probs(marg, cond).astype(np.float64)           # fp32 differences, as env_cell_prob forms them
    omega = et.solid_angles(MAP_W, MAP_H)
    pe_of = np.where(P > 0, P / omega, 0.0)
    # the bounce: sd = n + sphericalRand(1) of the RNG_SCATTER draw, bounce 0; it escapes (the floor is all there is)
    u = F.draw(seed_lo, seed_hi, pix, 0, 0, F.RNG_SCATTER)
    theta = F.u01(u[0]) * (2 * np.pi)
    z = F.u01(u[1]) * 2.0 - 1.0
    sp = np.sqrt(1.0 - z * z)
    sd = n + np.stack([sp * np.cos(theta), sp * np.sin(theta), z], axis=-1)
    wb = sd / np.linalg.norm(sd, axis=-1, keepdims=True)
    ib, jb, amb_b = lookup(wb)
    pb_b = wb[..., 1] / np.pi
    pe_b = pe_of[jb, ib]
    with np.errstate(divide="ignore", invalid="ignore"):
        w_b = np.where(pe_b > 0, pb_b ** 2 / (pb_b ** 2 + pe_b ** 2), 1.0)
    bounce = ALBEDO * L[jb, ib] * w_b
    default = ALBEDO * L[jb, ib]
    # the environment sample: RNG_ENV draw of (pixel, 0, 0)
    v = F.draw(seed_lo, seed_hi, pix, 0, 0, RNG_ENV)
    js = np.searchsorted(marg[1:], F.u01(v[0]).astype(np.float32), side="right")
    is_ = np.array([np.searchsorted(cond[j, 1:], x, side="right") for j, x in zip(js.ravel(), F.u01(v[1]).astype(np.float32).ravel())])
    is_ = is_.reshape(js.shape)
    assert (P[js, is_] > 0).all()                               # only cells of weight > 0 are drawn
    phi0, dphi, th0, _, dc = et.cells(MAP_W, MAP_H)
    phi = phi0[is_] + F.u01(v[2]) * dphi[is_]
    ct = np.cos(th0[js]) - F.u01(v[3]) * dc[js]
    we = et.directions(phi, ct)
    ie, je, amb_e = lookup(we)
    pb = ct / np.pi
    pe = pe_of[je, ie]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(pe > 0, pb * pe / (pb * pb + pe * pe), 0.0)
    env = ALBEDO * L[je, ie] * g
    return bounce + env, default, amb_b | amb_e | (is_ != ie) | (js != je), env


def test_env_nee_film_equals_the_float64_restatement(built, tmp_path):
    from hobbyraytracer_amd import api
    api.write_hdr(str(tmp_path / "block.hdr"), block_map())
    tex = api.read_hdr(str(tmp_path / "block.hdr"))
    table = api.env_table_build(tex)
    assert table is not None
    marg, cond = table
    path = os.path.join(str(tmp_path), "floor.yaml")
    with open(path, "w") as f:
        f.write(YAML)
    hs = api.HostScene(path, str(tmp_path))
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        cam = hs.camera(W, H)
        got, st = dev.render_tile(cam, api.default_params(W, H, 1, max_depth=2, seed=SEED, nee_env=True))
        def_got, st0 = dev.render_tile(cam, api.default_params(W, H, 1, max_depth=2, seed=SEED))
    finally:
        dev.close()
    film, default, amb, env_only = restate(tex, marg, cond, SEED & 0xFFFFFFFF, SEED >> 32)
    print(f"ambiguous fraction {amb.mean():.5f}, bounces into the block {int((default > 0).sum())} of {W * H}")
    assert amb.mean() < 0.02
    assert (default > 0).sum() > 100                  # the bounce's MIS weight is exercised, not only the environment sample
    assert st.rays == st0.rays == 2 * W * H
    assert W * H - amb.sum() <= st.shadow_rays <= W * H
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    ok = np.abs(got[..., 0] - film) <= 2e-4 * np.abs(film) + 1e-7
    bad = np.argwhere(~(ok | amb))
    assert bad.size == 0, [(tuple(i), got[tuple(i)][0], film[tuple(i)], env_only[tuple(i)]) for i in bad[:5]]
    okd = (np.abs(def_got[..., 0] - default) <= 2e-4 * np.abs(default) + 1e-7) | amb
    assert okd.all()
