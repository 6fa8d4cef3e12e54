"""Float64 pin of the stratified sampler (HRT_FLAG_STRATIFIED) inside a render: the scene of tests/test_gpu_nee_f64.py (a
Lambertian xz_rect floor under an xz_rect light, black background, max_depth 2, HRT_FLAG_NEE), samples 0..3 one by one.  Every pixel of
every sample is restated in numpy float64 from tests/stratified_np.py's restatement of the sampler (uint32 arithmetic, written from the
header's comment alone) and tests/f64_reference.py's primary_rays and rect_hit: the jitter is words x, y of the RNG_JITTER site, the
bounce sd = n + sphericalRand(1) of words x, y of the RNG_SCATTER site, the point on the light words y, z of the RNG_LIGHT site; p_l =
dist^2 / (A |cos|), p_b = cos / pi; the sample adds albedo Le p_b q / (p_b^2 + q^2) and the bounce albedo Le p_b^2 / (p_b^2 + q^2) when
it hits the light.  So which word of which site feeds which decision is pinned per sample, not only in distribution.
A bounce that meets the light within the ambiguity band of its edge may take either value; the band holds < 2 % of the samples."""
import os

import numpy as np
import pytest

from tests import f64_reference as F
from tests import stratified_np as SN

RNG_LIGHT = 6                  # hrt_rng.h
SEED = 0x0000123456789ABC
W, H = 64, 48
SAMPLES = 4
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


def restate(seed_lo, seed_hi, sample, draw):
    """sample `sample` of every pixel with the sampler `draw` (f64_reference.draw or stratified_np.draw)
    -> (NEE radiance, ambiguous mask, the light sample's term alone, the bounce hit the light), float64, [H, W, 3] / [H, W]"""
    cam = F.camera(CAM["look_from"], CAM["look_at"], CAM["up"], CAM["fov"], W / H)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pix = (py * W + px).astype(np.uint64)
    saved = F.draw
    F.draw = draw                       # primary_rays takes its jitter from the module's draw
    try:
        o, d = F.primary_rays(cam, W, H, px, py, sample, seed_lo, seed_hi)
    finally:
        F.draw = saved
    t, p, hit = F.rect_hit(o, d, 1, -50.0, 50.0, -50.0, 50.0, 0.0)
    assert hit.all() and (t > T_MIN).all()
    n = np.array([0.0, 1.0, 0.0])
    area = (2 * HALF) ** 2
    u = draw(seed_lo, seed_hi, pix, sample, 0, F.RNG_SCATTER)
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
    v = draw(seed_lo, seed_hi, pix, sample, 0, RNG_LIGHT)
    y = np.stack([-HALF + F.u01(v[1]) * (2 * HALF), np.full(px.shape, K_LIGHT), -HALF + F.u01(v[2]) * (2 * HALF)], axis=-1)
    dl = y - p
    dist2 = (dl ** 2).sum(-1)
    w = dl / np.sqrt(dist2)[..., None]
    pb = w[..., 1] / np.pi
    q = dist2 / (area * np.abs(w[..., 1]))
    g = pb * q / (pb * pb + q * q)
    nee = (ALBEDO * (w_b + g))[..., None] * LE
    delta = F.EPS * (1.0 + np.abs(yl[..., [0, 2]]).max(-1) + np.linalg.norm(yl - p, axis=-1))
    with np.errstate(invalid="ignore"):
        edge = np.minimum(np.abs(np.abs(yl[..., 0]) - HALF), np.abs(np.abs(yl[..., 2]) - HALF))
        amb = np.isfinite(tl) & (tl > 0) & (np.abs(yl[..., [0, 2]]).max(-1) < HALF + delta) & (edge < delta)
    return nee, amb, (ALBEDO * g)[..., None] * LE, hitl


def test_the_scene_stays_within_the_band_for_both_samplers():
    """no GPU: the ambiguity band of the pin holds < 2 % of the samples with the default sampler (the existing pin's own condition) and
    with the stratified one, and the bounce term is exercised"""
    for draw in (F.draw, SN.draw):
        amb, hits = [], 0
        for s in range(SAMPLES):
            _, a, _, hitl = restate(SEED & 0xFFFFFFFF, SEED >> 32, s, draw)
            amb.append(a.mean()); hits += int(hitl.sum())
        print(f"{draw.__module__}: ambiguous fraction {np.mean(amb):.5f}, bounce hits {hits} of {SAMPLES * W * H}")
        assert np.mean(amb) < 0.02 and hits > 20 * SAMPLES
    # the two samplers do not draw the same numbers
    assert not np.array_equal(restate(1, 0, 0, F.draw)[0], restate(1, 0, 0, SN.draw)[0])


@pytest.mark.gpu
def test_stratified_nee_samples_equal_the_float64_restatement(built, tmp_path):
    from hobbyraytracer_amd import api
    path = os.path.join(str(tmp_path), "floor.yaml")
    with open(path, "w") as f:
        f.write(YAML)
    hs = api.HostScene(path, str(tmp_path))
    dev = api.DeviceScene(hs.flat_ptr, 0)
    got = []
    try:
        cam = hs.camera(W, H)
        # one more sample than is rendered: no pass reaches the last one, so every pass leaves the plain sum of its one sample
        p = api.default_params(W, H, SAMPLES + 1, max_depth=2, seed=SEED, nee=True, stratified=True)
        for s in range(SAMPLES):
            acc = np.zeros((H, W, 3), np.float32)
            st = dev.render_stripes_accumulate(cam, p, 8, 0, 1, acc, s, 1)
            assert st.shadow_rays == W * H and st.rays == 2 * W * H, s
            got.append(acc)
    finally:
        dev.close()
    n_amb = 0
    for s in range(SAMPLES):
        nee, amb, direct_only, _ = restate(SEED & 0xFFFFFFFF, SEED >> 32, s, SN.draw)
        n_amb += int(amb.sum())
        ok = np.abs(got[s] - nee) <= 2e-4 * np.abs(nee) + 1e-7
        # inside the band the bounce may have missed: the light sample's term alone
        ok |= amb[..., None] & (np.abs(got[s] - direct_only) <= 2e-4 * np.abs(direct_only) + 1e-7)
        bad = np.argwhere(~ok.all(-1))
        assert bad.size == 0, (s, [(tuple(i), got[s][tuple(i)], nee[tuple(i)]) for i in bad[:5]])
        # ... and it is not the default sampler's film
        assert not np.allclose(got[s], restate(SEED & 0xFFFFFFFF, SEED >> 32, s, F.draw)[0], rtol=2e-4, atol=1e-7)
    print(f"ambiguous samples {n_amb} of {SAMPLES * W * H}")
    assert n_amb < 0.02 * SAMPLES * W * H
