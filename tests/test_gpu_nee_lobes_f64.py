"""Float64 pins of light sampling at metal and medium vertices (HRT_FLAG_NEE_LOBES): 1 spp, max_depth 2, black
background, every pixel restated in numpy float64 from tests/f64_reference.py's Philox, primary_rays, rect_hit and medium_free_path and
the definitions of DESIGN.md 4.8 alone.

(a) A metal xz_rect floor of roughness RHO < 1 (|m| = 1 / RHO > 1: two roots inside the lobe's cone) under an xz_rect light, seen at
    a grazing angle, so that the cone dips below the floor: bounces are absorbed and P_acc < 1.  The floor
    vertex (bounce 0) scatters sd = reflect(normalize(d), n) + RHO sphericalRand + eps with the RNG_SCATTER draw of (pixel, 0, 0); it
    survives when sd.y > 0.  A survivor samples the light through its RNG_LIGHT draw (words y, z the point): p_l = dist^2 / (A |cos|),
    p_b = the lobe's density of m = c / RHO, (t0^2 + t1^2) / (4 pi sqrt(D)) with D = 1 - |m x w|^2 (0 outside the cone: no shadow ray),
    and adds albedo Le p_b q / (p_b^2 + q^2) / P_acc (P_acc = min(1, (1 + m.y) / 2), the bounce's survival probability); its bounce adds albedo Le p_b^2 / (p_b^2 + q^2) when it hits the light.
(b) A sphere-bounded constant_medium under the light.  The camera segment's free path (RNG_MEDIUM draw of bounce 0) gives the vertex;
    the Isotropic scatter is ballRand (RNG_BALL attempts of bounce 0), p_b = 1 / (4 pi); the bounce's segment draws its free path with
    bounce 1 (a second medium hit ends the path at max_depth) and may reach the light; the light sample's shadow ray is
    d = cbrt(u01(word w of RNG_LIGHT)) w, whose own free path is drawn with the bounce field 0 | HRT_RNG_SHADOW.

Samples that may take either value -- a hit-or-miss within the band of the light's edge, of sd.y = 0 or of a free path against the
boundary -- and samples whose D lies within the band of the cone's edge, where p_b ~ 1 / sqrt(D) is not resolved to the tolerance by
fp32 (D carries ~16 ulp |m| of absolute error; 2e-4 on sqrt(D) needs D known to 4e-4: the band is D < 16 ulp |m| / 2e-4), are < 2 % of
the samples; the float64 restatement alone shows that share (printed).  `rays` and `shadow_rays` hang on signs only (sd.y, D), whose
own narrow bands hold no sample: they are asserted exactly.  (The unwrapped rects do not care for the shadow ray's length: the metal
length law rho t_k is witnessed by the brushed floor's wrapped mesh in tests/test_gpu_nee_lobes.py, not here.)"""
import os

import numpy as np
import pytest

from tests import f64_reference as F

pytestmark = pytest.mark.gpu

RNG_LIGHT = 6                  # hrt_rng.h
RNG_SHADOW = 0x80000000
SEED = 0x0000123456789ABC
SEED_A = 0x0000123456789ABD    # the metal pin: the first seed from SEED on whose sign bands (restate_metal `narrow`) hold no sample
W, H = 64, 48
T_MIN = 0.001
LE = np.array([0.9, 0.8, 0.7])
ULP = 2.0 ** -24

# ------------------------------------------------------------------ (a) the metal floor
ALBEDO, RHO = 0.5, 0.6
HALF, K_LIGHT = 0.5, 1.0
# a grazing view (45 - 80 degrees from the normal): the lobe's cone dips below the floor, m.y < 1 for most pixels (P_acc < 1) and a
# tenth of the bounces is absorbed
CAM_A = dict(look_from=(0.15, 0.5, 3.0), look_at=(0.15, -0.2, 2.0), up=(0.0, 1.0, 0.0), fov=36.0)


def _camera_yaml(cam, up):
    return f"""film:
    width: {W}
    height: {H}
    samples: 1
    output: out.png
camera:
    position: [{cam['look_from'][0]}, {cam['look_from'][1]}, {cam['look_from'][2]}]
    look_at: [{cam['look_at'][0]}, {cam['look_at'][1]}, {cam['look_at'][2]}]
    up: [{up[0]}, {up[1]}, {up[2]}]
    fov: {cam['fov']}
    aperture: 0
    focal_distance: 1
    background: [0, 0, 0]
"""


YAML_A = _camera_yaml(CAM_A, (0, 1, 0)) + f"""materials:
  - name: floor
    type: metal
    albedo: [{ALBEDO}, {ALBEDO}, {ALBEDO}]
    roughness: {RHO}
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


def _sphere_rand(u):
    """hrt_rng.h spherical_rand of words x, y"""
    theta = F.u01(u[0]) * (2 * np.pi)
    z = F.u01(u[1]) * 2.0 - 1.0
    sp = np.sqrt(1.0 - z * z)
    return np.stack([sp * np.cos(theta), sp * np.sin(theta), z], axis=-1)


def _lobe_pdf(m, w):
    """-> (p_b, D) of the unit direction w for the lobe m = c / rho"""
    c = (w * m).sum(-1)
    x = np.cross(m, w)
    D = 1.0 - (x * x).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        sD = np.sqrt(np.maximum(D, 0.0))
        big = np.where(c >= 0, c + sD, c - sD)
        other = ((m * m).sum(-1) - 1.0) / big
        t0, t1 = np.maximum(big, 0.0), np.maximum(other, 0.0)
        pb = np.where(D > 0, (t0 * t0 + t1 * t1) / (4 * np.pi * sD), 0.0)
    return pb, D


def _light_sample(seed_lo, seed_hi, pix, p, k=K_LIGHT):
    """the RNG_LIGHT draw of (pixel, sample 0, bounce 0): words y / z = the point of the light, P_sel = 1 -> (w, q, dist, word w)"""
    v = F.draw(seed_lo, seed_hi, pix, 0, 0, RNG_LIGHT)
    y = np.stack([-HALF + F.u01(v[1]) * (2 * HALF), np.full(pix.shape, k), -HALF + F.u01(v[2]) * (2 * HALF)], axis=-1)
    dl = y - p
    dist2 = (dl ** 2).sum(-1)
    w = dl / np.sqrt(dist2)[..., None]
    q = dist2 / ((2 * HALF) ** 2 * np.abs(w[..., 1]))
    return w, q, np.sqrt(dist2), v[3]


def _light_hit(p, sd, k=K_LIGHT):
    """the bounce's segment against the light -> (hit, q of its direction, ambiguous at the light's edge)"""
    tl, yl, hitl = F.rect_hit(p, sd, 1, -HALF, HALF, -HALF, HALF, k)
    hitl &= tl >= T_MIN
    wl = sd / np.linalg.norm(sd, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ((yl - p) ** 2).sum(-1) / ((2 * HALF) ** 2 * np.abs(wl[..., 1]))
        delta = F.EPS * (1.0 + np.abs(yl[..., [0, 2]]).max(-1) + np.linalg.norm(yl - p, axis=-1))
        edge = np.minimum(np.abs(np.abs(yl[..., 0]) - HALF), np.abs(np.abs(yl[..., 2]) - HALF))
        amb = np.isfinite(tl) & (tl > 0) & (np.abs(yl[..., [0, 2]]).max(-1) < HALF + delta) & (edge < delta)
    return hitl, q, amb


def _mis(pb, q):
    with np.errstate(divide="ignore", invalid="ignore"):
        s = pb * pb + q * q
        return np.where(s > 0, pb * pb / s, 0.0), np.where(s > 0, pb * q / s, 0.0)


def restate_metal(seed_lo, seed_hi):
    cam = F.camera(CAM_A["look_from"], CAM_A["look_at"], CAM_A["up"], CAM_A["fov"], W / H)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pix = (py * W + px).astype(np.uint64)
    o, d = F.primary_rays(cam, W, H, px, py, 0, seed_lo, seed_hi)
    t, p, hit = F.rect_hit(o, d, 1, -50.0, 50.0, -50.0, 50.0, 0.0)
    assert hit.all() and (t > T_MIN).all()
    n = np.array([0.0, 1.0, 0.0])
    v = d / np.linalg.norm(d, axis=-1, keepdims=True)
    c = v - 2.0 * (v * n).sum(-1)[..., None] * n + 2.0 ** -23
    m = c / RHO
    r = np.linalg.norm(m, axis=-1)
    sd = (v - 2.0 * (v * n).sum(-1)[..., None] * n) + RHO * _sphere_rand(F.draw(seed_lo, seed_hi, pix, 0, 0, F.RNG_SCATTER)) + 2.0 ** -23
    surv = sd[..., 1] > 0
    amb = np.abs(sd[..., 1]) < F.EPS * 2.0
    cone_band = 16 * ULP * r / 2e-4
    # the bounce
    wb = sd / np.linalg.norm(sd, axis=-1, keepdims=True)
    pb_b, D_b = _lobe_pdf(m, wb)
    hit_b, q_b, amb_edge = _light_hit(p, sd)
    w_b, _ = _mis(pb_b, q_b)
    amb |= amb_edge
    skip = surv & ((hit_b & (D_b < cone_band)) | (D_b < 16 * ULP * r))     # the weight's p_b, or whether the vertex is eligible at all
    # the light sample
    w, q, _, _ = _light_sample(seed_lo, seed_hi, pix, p)
    pb, D = _lobe_pdf(m, w)
    skip |= surv & (np.abs(D) < cone_band)
    _, g = _mis(pb, q)
    p_acc = np.minimum(1.0, 0.5 * (1.0 + m[..., 1]))             # the survival probability of the vertex's own bounce
    g = np.where(w[..., 1] > 0, g, 0.0) / p_acc                 # the acceptance dot(w, nn) > 0 (the lamp is above the floor: always)
    shadow = surv & (pb > 0) & (w[..., 1] > 0)
    # whether a shadow ray is cast at all hangs on the SIGN of D (light sample) and of D_b (the vertex's eligibility), and `rays` on the
    # sign of sd.y: their own narrow bands, not the wide one where 1 / sqrt(D) is unresolved
    narrow = (np.abs(sd[..., 1]) < F.EPS * 2.0) | (surv & ((np.abs(D) < 16 * ULP * r) | (D_b < 16 * ULP * r)))
    nee = (ALBEDO * surv * (np.where(hit_b, w_b, 0.0) + g))[..., None] * LE
    default = (ALBEDO * (surv & hit_b))[..., None] * LE
    # either value inside the hit-or-miss bands: the bounce's term may be absent (or, at sd.y = 0, everything)
    alt = [(ALBEDO * surv * g)[..., None] * LE, np.zeros_like(nee)]
    c_l = (w * m).sum(-1)
    two_roots = shadow & (c_l - np.sqrt(np.maximum(D, 0.0)) > 0)          # both roots of |t w - m| = 1 positive
    return dict(nee=nee, default=default, amb=amb, skip=skip, alt=alt, shadow=shadow, surv=surv, two_roots=two_roots, hit_b=surv & hit_b,
                narrow=narrow, p_acc=p_acc, no_acc=(ALBEDO * surv * (np.where(hit_b, w_b, 0.0) + g * p_acc))[..., None] * LE)


# ------------------------------------------------------------------ (b) the medium
SIGMA, FOG = 1.0, np.array([0.9, 0.6, 0.4])
BALL = ((0.0, 0.0, 0.0), 1.0)
K_LIGHT_B = 2.5
CAM_B = dict(look_from=(0.0, 0.0, 4.0), look_at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=30.0)
YAML_B = _camera_yaml(CAM_B, (0, 1, 0)) + f"""materials:
  - name: lamp
    type: diffuse_light
    albedo: [{LE[0]}, {LE[1]}, {LE[2]}]
    strength: 1
objects:
  - type: constant_medium
    density: {SIGMA}
    colour: [{FOG[0]}, {FOG[1]}, {FOG[2]}]
    boundary:
        type: sphere
        center: [0, 0, 0]
        radius: 1
  - type: xz_rect
    x: [{-HALF}, {HALF}]
    z: [{-HALF}, {HALF}]
    k: {K_LIGHT_B}
    material: lamp
"""


def restate_medium(seed_lo, seed_hi):
    cam = F.camera(CAM_B["look_from"], CAM_B["look_at"], CAM_B["up"], CAM_B["fov"], W / H)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pix = (py * W + px).astype(np.uint64)
    o, d = F.primary_rays(cam, W, H, px, py, 0, seed_lo, seed_hi)
    assert not F.rect_hit(o, d, 1, -HALF - 0.1, HALF + 0.1, -HALF - 0.1, HALF + 0.1, K_LIGHT_B)[2].any()   # the lamp is out of view
    sigma = np.float64(np.float32(SIGMA))
    med_u = lambda bounce: F.u01(F.draw(seed_lo, seed_hi, pix, 0, bounce, F.RNG_MEDIUM, 0)[0])   # noqa: E731  (the medium is prim 0)
    # the camera segment
    t, _, amb0 = F.medium_free_path("sphere", BALL, sigma, o, d, T_MIN, np.inf, med_u(0))
    vert = np.isfinite(t)
    x = o + np.where(vert, t, 0.0)[..., None] * d
    # the Isotropic scatter: ballRand's rejection loop, RNG_BALL attempt k of bounce 0
    sd = np.zeros(x.shape)
    todo = np.ones(pix.shape, bool)
    amb_ball = np.zeros(pix.shape, bool)
    for attempt in range(64):
        u = F.draw(seed_lo, seed_hi, pix, 0, 0, F.RNG_BALL, attempt)
        cand = np.stack([F.u01(u[k]) * 2.0 - 1.0 for k in range(3)], axis=-1)
        ln = np.linalg.norm(cand, axis=-1)
        amb_ball |= todo & (np.abs(ln - 1.0) < F.EPS)
        take = todo & ~(ln > 1.0)
        sd[take] = cand[take]
        todo &= ~take
        if not todo.any():
            break
    # the bounce's segment (bounce 1): a second medium hit ends the path at max_depth; otherwise the lamp or nothing
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, _, amb1 = F.medium_free_path("sphere", BALL, sigma, x, sd, T_MIN, np.inf, med_u(1))
    hit_b, q_b, amb_edge = _light_hit(x, sd, K_LIGHT_B)
    hit_b &= ~np.isfinite(t1)
    # the light sample: d = cbrt(u) w, its free path drawn with the bounce field 0 | HRT_RNG_SHADOW
    w, q, dist, word_w = _light_sample(seed_lo, seed_hi, pix, x, K_LIGHT_B)
    ln = np.cbrt(F.u01(word_w))
    ds = ln[..., None] * w
    with np.errstate(divide="ignore", invalid="ignore"):
        ts, _, amb_s = F.medium_free_path("sphere", BALL, sigma, x, ds, T_MIN, dist / ln * 1.001, med_u(RNG_SHADOW))
    seen = ~np.isfinite(ts)
    pb = 1.0 / (4.0 * np.pi)
    w_b, _ = _mis(pb, q_b)
    _, g = _mis(pb, q)
    shadow = vert & (ln > 0)
    nee = (vert * (np.where(hit_b, w_b, 0.0) + np.where(seen & shadow, g, 0.0)))[..., None] * LE * FOG
    default = (vert & hit_b)[..., None] * LE * FOG
    amb = amb0 | (vert & (amb_ball | amb1 | amb_edge | amb_s))
    second = vert          # every vertex traces its bounce's segment
    return dict(nee=nee, default=default, amb=amb, shadow=shadow, second=second, seen=vert & seen, hit_b=vert & hit_b)


def _render(tmp_path, name, yaml, seed=SEED):
    from hobbyraytracer_amd import api
    path = os.path.join(str(tmp_path), name + ".yaml")
    with open(path, "w") as f:
        f.write(yaml)
    hs = api.HostScene(path, str(tmp_path))
    dev = api.DeviceScene(hs.flat_ptr, 0)
    try:
        cam = hs.camera(W, H)
        got, st = dev.render_tile(cam, api.default_params(W, H, 1, max_depth=2, seed=seed, nee_lobes=True))
        nee_only, st_n = dev.render_tile(cam, api.default_params(W, H, 1, max_depth=2, seed=seed, nee=True))
        def_got, st0 = dev.render_tile(cam, api.default_params(W, H, 1, max_depth=2, seed=seed))
    finally:
        dev.close()
    return got, st, nee_only, st_n, def_got, st0


def _close(a, b):
    return (np.abs(a - b) <= 2e-4 * np.abs(b) + 1e-7).all(-1)


def test_metal_floor_film_equals_the_float64_restatement(built, tmp_path):
    r = restate_metal(SEED_A & 0xFFFFFFFF, SEED_A >> 32)
    unsure = r["amb"] | r["skip"]
    lowered = r["shadow"] & (r["p_acc"] < 0.999)
    print(f"metal floor: ambiguous or unresolved fraction {unsure.mean():.5f} (hit-or-miss {r['amb'].mean():.5f}, cone edge {r['skip'].mean():.5f}); "
          f"survivors {int(r['surv'].sum())}, light samples inside the cone {int(r['shadow'].sum())} ({int(r['two_roots'].sum())} with two roots, "
          f"{int(lowered.sum())} at P_acc < 1, min P_acc {r['p_acc'][r['shadow']].min():.3f}), bounce hits {int(r['hit_b'].sum())} of {W * H}; "
          f"sign bands hold {int(r['narrow'].sum())}")
    assert unsure.mean() < 0.02
    assert r["narrow"].sum() == 0                          # no count below can go either way
    # every branch is exercised: absorbed bounces, light samples outside the cone, two-root directions, P_acc < 1
    assert r["hit_b"].sum() > 20 and r["shadow"].sum() > 200 and (r["surv"] & ~r["shadow"]).sum() > 20
    assert (~r["surv"]).sum() > 100 and r["two_roots"].sum() > 200 and lowered.sum() > 200
    got, st, nee_only, st_n, def_got, st0 = _render(tmp_path, "metal_floor", YAML_A, SEED_A)
    print(f"rays {st.rays}, shadow_rays {st.shadow_rays}")
    assert st.rays == st0.rays == st_n.rays == W * H + int(r["surv"].sum())
    assert st.shadow_rays == int(r["shadow"].sum())
    assert st_n.shadow_rays == 0 and np.array_equal(nee_only.view(np.uint32), def_got.view(np.uint32))   # --nee alone: no eligible vertex
    ok = _close(got, r["nee"]) | r["skip"]
    for alt in r["alt"]:
        ok |= r["amb"] & _close(got, alt)
    bad = np.argwhere(~ok)
    assert bad.size == 0, [(tuple(i), got[tuple(i)], r["nee"][tuple(i)]) for i in bad[:5]]
    assert (_close(def_got, r["default"]) | r["amb"]).all()
    sure = ~unsure
    assert (np.abs(got - def_got).max(-1)[sure] > 0).sum() > 200         # the flag changes the film
    # ... and the film is NOT the one without the division by P_acc, wherever P_acc < 1 and the light sample counts
    assert (~_close(got, r["no_acc"]))[sure & lowered].mean() > 0.95


def test_medium_film_equals_the_float64_restatement(built, tmp_path):
    r = restate_medium(SEED & 0xFFFFFFFF, SEED >> 32)
    print(f"medium: ambiguous fraction {r['amb'].mean():.5f}; vertices {int(r['second'].sum())}, lamp seen by {int(r['seen'].sum())} shadow rays, "
          f"bounce hits {int(r['hit_b'].sum())} of {W * H}")
    assert r["amb"].mean() < 0.02
    assert r["seen"].sum() > 200 and (r["shadow"] & ~r["seen"]).sum() > 200 and r["hit_b"].sum() > 5
    got, st, nee_only, st_n, def_got, st0 = _render(tmp_path, "medium", YAML_B)
    n_amb = int(r["amb"].sum())
    print(f"rays {st.rays} (restated {W * H + int(r['second'].sum())}), shadow_rays {st.shadow_rays} (restated {int(r['shadow'].sum())}), ambiguous {n_amb}")
    assert st.rays == st0.rays == st_n.rays
    assert st_n.shadow_rays == 0 and np.array_equal(nee_only.view(np.uint32), def_got.view(np.uint32))
    assert abs(st.rays - (W * H + int(r["second"].sum()))) <= n_amb
    assert abs(st.shadow_rays - int(r["shadow"].sum())) <= n_amb
    if n_amb == 0:
        assert st.rays == W * H + int(r["second"].sum()) and st.shadow_rays == int(r["shadow"].sum())
    ok = _close(got, r["nee"]) | r["amb"]
    bad = np.argwhere(~ok)
    assert bad.size == 0, [(tuple(i), got[tuple(i)], r["nee"][tuple(i)]) for i in bad[:5]]
    assert (_close(def_got, r["default"]) | r["amb"]).all()
