"""Pin of Russian roulette (HRT_FLAG_ROULETTE) inside a render, decision by decision: the floor under a rect light of
tests/test_gpu_stratified.py (a Lambertian xz_rect of albedo 0.5 under an xz_rect light, black background), without next-event
estimation, max_depth 2, first_bounce 0, samples 0..3 one by one.  Every camera ray meets the floor and scatters with attenuation 0.5, so
q = 0.5 at vertex 0 of every path, whatever the floor parameter's 0.05 says.  The coin is restated in numpy from tests/f64_reference.py's
Philox (and, under HRT_FLAG_STRATIFIED, tests/stratified_np.py's sampler): u = u01(word x of the RNG_ROULETTE site of (pixel, sample,
bounce 0)); u >= 0.5 kills.  A killed pixel must be exactly 0; a surviving one exactly the default render's value of that sample divided by
q -- a power of two, so bit for bit.  Vertex 1, if the bounce reaches it, is the light (no scatter, no roulette) or the floor at the depth
limit (ended before the rule).
The ambiguity band of the float64 pins (a bounce that meets the light within BAND_ULPS of its edge) does not enter the comparison -- both
renders trace the same path -- but the scene must stay as clear of it as those pins ask: < 2 % of the samples."""
import numpy as np
import pytest

from tests import f64_reference as F
from tests import stratified_np as SN
from tests.test_gpu_stratified import ALBEDO, FLOOR_YAML, HALF, H_LIGHT, _scene

RNG_ROULETTE = 8               # hrt_rng.h
SEED = 0x00000BADC0FFEE11
W = H = 32                     # the film of FLOOR_YAML
SAMPLES = 4
Q = 0.5
CAM = dict(look_from=(0.1, 0.6, 0.05), look_at=(0.1, 0.0, 0.0501), up=(0.0, 0.0, -1.0), fov=60.0)      # FLOOR_YAML's camera


def predict_killed(sample, draw):
    """[H, W] bool: the path of (pixel, sample) ends at vertex 0"""
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pix = (py * W + px).astype(np.uint64)
    u = F.u01(draw(SEED & 0xFFFFFFFF, SEED >> 32, pix, sample, 0, RNG_ROULETTE)[0])
    return u >= Q


def band_fraction(sample, draw):
    """the share of this sample's bounces that meet the light within the ambiguity band of its edge, and the number that hit it"""
    cam = F.camera(CAM["look_from"], CAM["look_at"], CAM["up"], CAM["fov"], W / H)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pix = (py * W + px).astype(np.uint64)
    saved = F.draw
    F.draw = draw                       # primary_rays takes its jitter from the module's draw
    try:
        o, d = F.primary_rays(cam, W, H, px, py, sample, SEED & 0xFFFFFFFF, SEED >> 32)
    finally:
        F.draw = saved
    t, p, hit = F.rect_hit(o, d, 1, -50.0, 50.0, -50.0, 50.0, 0.0)
    assert hit.all() and (t > 0.001).all()
    u = draw(SEED & 0xFFFFFFFF, SEED >> 32, pix, sample, 0, F.RNG_SCATTER)
    theta = F.u01(u[0]) * (2 * np.pi)
    z = F.u01(u[1]) * 2.0 - 1.0
    sp = np.sqrt(1.0 - z * z)
    sd = np.array([0.0, 1.0, 0.0]) + np.stack([sp * np.cos(theta), sp * np.sin(theta), z], axis=-1)
    tl, yl, hitl = F.rect_hit(p, sd, 1, -HALF, HALF, -HALF, HALF, H_LIGHT)
    delta = F.EPS * (1.0 + np.abs(yl[..., [0, 2]]).max(-1) + np.linalg.norm(yl - p, axis=-1))
    with np.errstate(invalid="ignore"):
        edge = np.minimum(np.abs(np.abs(yl[..., 0]) - HALF), np.abs(np.abs(yl[..., 2]) - HALF))
        amb = np.isfinite(tl) & (tl > 0) & (np.abs(yl[..., [0, 2]]).max(-1) < HALF + delta) & (edge < delta)
    return float(amb.mean()), int((hitl & (tl >= 0.001)).sum())


def test_the_scene_is_what_the_pin_assumes():
    """no GPU: albedo 0.5 makes q a power of two; both samplers' coins kill about half the paths and not the same ones; the band
    holds < 2 % of the samples and some bounces do reach the light"""
    assert ALBEDO == Q
    for draw in (F.draw, SN.draw):
        frac = np.mean([predict_killed(s, draw).mean() for s in range(SAMPLES)])
        amb, hits = zip(*[band_fraction(s, draw) for s in range(SAMPLES)])
        print(f"{draw.__module__}: killed fraction {frac:.4f}, ambiguous fraction {np.mean(amb):.5f}, bounce hits {sum(hits)} of {SAMPLES * W * H}")
        assert 0.4 < frac < 0.6 and np.mean(amb) < 0.02 and sum(hits) > 10 * SAMPLES
    assert not np.array_equal(predict_killed(0, F.draw), predict_killed(0, SN.draw))
    assert not np.array_equal(predict_killed(0, F.draw), predict_killed(1, F.draw))


@pytest.mark.gpu
@pytest.mark.parametrize("stratified", [False, True], ids=["philox", "stratified"])
def test_every_decision_at_vertex_0_is_the_predicted_one(built, tmp_path, stratified):
    from hobbyraytracer_amd import api
    hs = _scene(tmp_path, "floor", FLOOR_YAML)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    draw = SN.draw if stratified else F.draw
    try:
        dev.set_roulette(0, 0.05)
        cam = hs.camera(W, H)
        # one more sample than is rendered: no pass reaches the last one, so every pass leaves the plain sum of its one sample
        base = api.default_params(W, H, SAMPLES + 1, max_depth=2, seed=SEED, stratified=stratified)
        rr = api.default_params(W, H, SAMPLES + 1, max_depth=2, seed=SEED, stratified=stratified, roulette=True)
        n_killed = n_lit = 0
        for s in range(SAMPLES):
            plain, got = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
            st0 = dev.render_stripes_accumulate(cam, base, 8, 0, 1, plain, s, 1)
            st1 = dev.render_stripes_accumulate(cam, rr, 8, 0, 1, got, s, 1)
            killed = predict_killed(s, draw)
            assert st0.rays == 2 * W * H and st1.rays == 2 * W * H - int(killed.sum()), (s, st0.rays, st1.rays, int(killed.sum()))
            assert (got[killed].view(np.uint32) == 0).all(), (s, "a killed path left radiance, or was not killed")
            want = plain / np.float32(Q)                                     # exact: a power of two
            assert np.array_equal(got[~killed].view(np.uint32), want[~killed].view(np.uint32)), s
            n_killed += int(killed.sum()); n_lit += int((got.sum(-1) > 0).sum())
        amb = [band_fraction(s, draw)[0] for s in range(SAMPLES)]
        print(f"stratified={stratified}: {n_killed} of {SAMPLES * W * H} paths killed at vertex 0, {n_lit} surviving samples carry light, "
              f"ambiguous fraction {np.mean(amb):.5f}")
        assert n_lit > 10 * SAMPLES                                          # the comparison is not 0 == 0 throughout
        assert np.mean(amb) < 0.02
    finally:
        dev.close()
