"""The guided denoiser (include/hrt.h "guided denoiser") without a GPU: the C ABI is declared, exported, bound and still
C99; bad arguments are refused before any device is touched with the output untouched; the numpy restatement of the header's words
(tests/denoise_np.py) has the properties an edge-avoiding filter must have; and it lowers the error of a noisy oracle film against a
converged one on two scenes -- the quality test, decided here because GPU films are the oracle's bits (tests/test_gpu_denoise.py
requires the kernels to give the restatement's bits)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import denoise_np as dn
from tests.test_abi import ROOT, _declared_functions

DENOISE_SYMBOLS = ("hrt_denoise_defaults", "hrt_denoise_workspace_bytes", "hrt_denoise_device", "hrt_denoise", "hrt_denoise_resolve_u8")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the C ABI
def test_the_symbols_are_declared_exported_and_bound(built):
    from hobbyraytracer_amd import api
    declared = _declared_functions("hrt.h")
    lib = C.CDLL(api.HIP_LIB_PATH)
    for name in DENOISE_SYMBOLS:
        assert name in declared, f"include/hrt.h does not declare {name}"
        assert hasattr(lib, name), f"libhrt_hip.so does not export {name}"
        assert name in api.HIP_SYMBOLS
    for f in (api.denoise, api.denoise_device, api.denoise_defaults, api.denoise_workspace_bytes, api.denoise_resolve_u8):
        assert callable(f)
    p = api.denoise_defaults()
    assert {n: getattr(p, n) for n, _ in api.DenoiseParams._fields_} == {k: (np.float32(v) if isinstance(v, float) else v) for k, v in dn.DEFAULTS.items()}
    assert api.denoise_workspace_bytes(640, 640) == 48 * 640 * 640
    assert api.denoise_workspace_bytes(0, 5) == 0 and api.denoise_workspace_bytes(1 << 16, 1 << 15) == 0 and api.denoise_workspace_bytes(1 << 15, 1 << 15) == 48 << 30


def test_the_header_is_c99_and_the_params_struct_has_the_size_of_its_ctypes_twin(built, tmp_path):
    from hobbyraytracer_amd import api
    src = tmp_path / "dn.c"
    src.write_text('#include <stdio.h>\n' f'#include "{ROOT}/include/hrt.h"\n'
                   "void (*a)(hrt_denoise_params*) = hrt_denoise_defaults;\n"
                   "uint64_t (*b)(int32_t, int32_t) = hrt_denoise_workspace_bytes;\n"
                   "hrt_status (*c)(int, int32_t, int32_t, const hrt_denoise_params*, const float*, const float*, const float*, float*, void*, void*) = "
                   "hrt_denoise_device;\n"
                   "hrt_status (*d)(int, int32_t, int32_t, const hrt_denoise_params*, const float*, const float*, const float*, float*) = hrt_denoise;\n"
                   "hrt_status (*e)(int, const float*, int64_t, uint8_t*) = hrt_denoise_resolve_u8;\n"
                   'int main(void){ printf("%d\\n", (int)sizeof(hrt_denoise_params)); return a && b && c && d && e ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-o", str(tmp_path / "dn.o"), str(src)])
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "dn"), str(src), "-L" + api.LIB_DIR, "-lhrt_hip", "-Wl,-rpath," + api.LIB_DIR,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert int(subprocess.check_output([str(tmp_path / "dn")]).decode()) == C.sizeof(api.DenoiseParams) == 20


def test_bad_arguments_are_refused_before_any_device_is_touched_and_leave_the_output_untouched(built):
    from hobbyraytracer_amd import api
    W, H = 8, 6
    rgb, aov, var = np.ones((H, W, 3), np.float32), np.ones((H, W, 8), np.float32), np.ones((H, W), np.float32)
    out = np.full((H, W, 3), 7.0, np.float32)
    ws = np.zeros(api.denoise_workspace_bytes(W, H) // 4 + 8, np.float32)
    ws_ptr = (ws.ctypes.data + 15) & ~15
    aov_ok = aov.ctypes.data % 16 == 0
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    vp = lambda a: C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a)      # noqa: E731
    good = api.denoise_defaults()

    def host(p=good, w=W, h=H, r=rgb, a=aov, v=var, o=out):
        return api._hip.hrt_denoise(0, w, h, C.byref(p) if p is not None else None, fp(r) if r is not None else None,
                                    fp(a) if a is not None else None, fp(v) if v is not None else None, fp(o) if o is not None else None)

    def device(p=good, w=W, h=H, r=rgb, a=aov, v=var, o=out, s=ws_ptr):
        return api._hip.hrt_denoise_device(0, w, h, C.byref(p) if p is not None else None, vp(r) if r is not None else None,
                                           vp(a) if a is not None else None, vp(v) if v is not None else None, vp(o) if o is not None else None,
                                           C.c_void_p(s) if s else None, None)

    def refused(st, word):
        assert st == api.HRT_ERR_INVALID, (st, word)
        assert word.encode() in api._hip.hrt_last_error(), (word, api._hip.hrt_last_error())
        assert (out == 7.0).all()

    for call in (host, device):
        for missing in ("p", "r", "a", "o"):
            refused(call(**{missing: None}), "NULL")
        refused(call(w=0), "width")
        refused(call(h=-3), "width")
        refused(call(w=1 << 16, h=(1 << 14) + 1), "2^30")
        bad = {"iterations": (0, 9, -1), "normal_squarings": (-1, 11), "sigma_l": (0.0, -1.0, float("nan"), float("inf")),
               "sigma_z": (0.0, -2.0, float("nan"), float("inf")), "albedo_floor": (0.0, -0.5, float("nan"), float("inf"))}
        for field, values in bad.items():
            for v in values:
                refused(call(p=api.denoise_defaults(**{field: v})), field)
    refused(device(s=None), "NULL")
    refused(device(s=ws_ptr + 4), "misaligned")
    if aov_ok:
        refused(api._hip.hrt_denoise_device(0, W, H, C.byref(good), vp(rgb), C.c_void_p(aov.ctypes.data + 8), None, vp(out), C.c_void_p(ws_ptr), None), "misaligned")
    refused(api._hip.hrt_denoise_device(0, W, H, C.byref(good), C.c_void_p(rgb.ctypes.data + 2), vp(aov), None, vp(out), C.c_void_p(ws_ptr), None), "misaligned")
    # the Python wrapper checks the shapes itself
    with pytest.raises(ValueError):
        api.denoise(rgb, aov[:, :, :7])
    with pytest.raises(ValueError):
        api.denoise(rgb, aov, variance=var[:, :4])
    with pytest.raises(TypeError):
        api.denoise_defaults(sigma_x=1.0)


# ---------------------------------------------------------------- properties of the restatement
def _guides(H, W, albedo=(0.7, 0.5, 0.3), normal=(0.0, 0.0, 1.0), depth=4.0):
    aov = np.zeros((H, W, 8), np.float32)
    aov[..., 0:3] = albedo
    aov[..., 3] = 1.0
    aov[..., 4:7] = normal
    aov[..., 7] = depth
    return aov


def _noisy(H, W, seed, level=(0.4, 0.3, 0.2), amp=0.15):
    r = np.random.default_rng(seed)
    return (np.array(level, np.float32) + amp * r.standard_normal((H, W, 3))).astype(np.float32)


def test_a_constant_image_comes_back_within_2_ulp():
    H, W = 21, 34
    rgb = np.empty((H, W, 3), np.float32)
    rgb[...] = (0.37, 1.9, 0.052)
    for var in (None, np.full((H, W), 0.01, np.float32)):
        out = dn.denoise(rgb, _guides(H, W), var)
        ulp = np.abs(out.view(np.int32).astype(np.int64) - rgb.view(np.int32).astype(np.int64))
        assert ulp.max() <= 2, ulp.max()


def _exact_variance(aov, target=2.0 ** -6):
    """A given variance whose prepared v is the power of two `target` in every pixel of a film of one albedo: every partial sum of the
    3 x 3 mean of v is then exact, so that mean is `target` whichever neighbours are present."""
    af = aov[0, 0, 0:3]
    ya = dn.lum(af[0], af[1], af[2])
    var = np.float32(target) * (ya * ya)
    for _ in range(64):
        if var / (ya * ya) == np.float32(target):
            break
        var = np.nextafter(var, np.float32(np.inf) if var / (ya * ya) < target else np.float32(0))
    assert var / (ya * ya) == np.float32(target)
    return np.full(aov.shape[:2], var, np.float32)


def _check_sides_never_mix(rgb, aov, left):
    """Two statements of "the sides never mix".  (1) Bit for bit: with one iteration and a given variance that is the same exact power
    of two everywhere (so that the 3 x 3 mean of v, the one quantity the definition lets cross an edge, is the same number with or
    without the other side), each side equals a filter run of that side alone -- the other side's pixels invalid, i.e. absent.  (2) With
    the default parameters and the spatial variance estimate every output value of a side lies inside the range of that side's own
    input (2 ulp for the roundings of a weighted mean and of e * af): no weight, however small, reaches across."""
    var = _exact_variance(aov)
    whole = dn.denoise(rgb, aov, var, iterations=1)
    assert not np.array_equal(whole, rgb)
    for mask in (left, ~left):
        alone = rgb.copy()
        alone[~mask] = np.nan
        assert np.array_equal(_bits(whole[mask]), _bits(dn.denoise(alone, aov, var, iterations=1)[mask]))
    out = dn.denoise(rgb, aov)
    for mask in (left, ~left):
        lo, hi = rgb[mask].min(axis=0), rgb[mask].max(axis=0)
        slack = 2 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)))
        assert (out[mask] >= lo - slack).all() and (out[mask] <= hi + slack).all()
        assert (out[mask].std(axis=0) < rgb[mask].std(axis=0)).all()                 # ... while each side is smoothed


def test_two_half_planes_with_different_normals_never_mix():
    H, W = 24, 40
    rgb = _noisy(H, W, 1)
    rgb[:, 23:] += np.float32(1.5)
    aov = _guides(H, W)
    left = np.zeros((H, W), bool)
    left[:, :23] = True
    aov[~left, 4:7] = (1.0, 0.0, 0.0)            # perpendicular: the cosine is exactly 0
    _check_sides_never_mix(rgb, aov, left)


def test_a_depth_step_beyond_sigma_z_never_mixes():
    H, W = 24, 40
    rgb = _noisy(H, W, 2)
    rgb[11:] += np.float32(1.5)
    aov = _guides(H, W)
    left = np.zeros((H, W), bool)
    left[:11] = True
    aov[~left, 7] = 9.0                          # |4 - 9| / (0.5 * 9) > 1
    _check_sides_never_mix(rgb, aov, left)
    near = aov.copy()
    near[~left, 7] = 4.5                         # within sigma_z, on a film without the step in radiance: the sides do mix
    flat = _noisy(H, W, 2)
    assert not np.array_equal(_bits(dn.denoise(flat, near)[left]), _bits(dn.denoise(flat, aov)[left]))


def test_an_invalid_pixel_keeps_its_bits_and_moves_no_neighbour():
    H, W = 19, 23
    rgb = _noisy(H, W, 3)
    aov = _guides(H, W)
    bad = rgb.copy()
    payload = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
    bad[7, 9] = (payload, 0.3, 0.2)
    bad[12, 3] = (0.1, np.inf, 0.2)
    bad[0, 0] = (0.1, 0.2, -np.inf)
    out = dn.denoise(bad, aov)
    for y, x in ((7, 9), (12, 3), (0, 0)):
        assert np.array_equal(_bits(out[y, x]), _bits(bad[y, x]))
    assert np.isfinite(np.delete(out.reshape(-1, 3), [7 * W + 9, 12 * W + 3, 0], axis=0)).all()
    # ... and the rest is what the filter gives when those pixels hold any other non-finite value
    other = rgb.copy()
    for y, x in ((7, 9), (12, 3), (0, 0)):
        other[y, x] = np.nan
    ref = dn.denoise(other, aov)
    ok = np.isfinite(bad).all(axis=-1)
    assert np.array_equal(_bits(out[ok]), _bits(ref[ok]))


def test_zero_variance_given_leaves_a_noisy_image_unchanged():
    H, W = 20, 27
    rgb = _noisy(H, W, 4)
    aov = _guides(H, W)
    e = rgb / aov[..., 0:3]
    l = dn.lum(e[..., 0], e[..., 1], e[..., 2])
    # every pair of pixels a tap can join differs by more than 1e-6 in luminance (true of this seed; asserted, not assumed)
    for s in (1, 2, 4, 8, 16):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if (dx or dy) and abs(dx * s) < W and abs(dy * s) < H:
                    a = l[max(0, dy * s):H + min(0, dy * s), max(0, dx * s):W + min(0, dx * s)]
                    b = l[max(0, -dy * s):H + min(0, -dy * s), max(0, -dx * s):W + min(0, -dx * s)]
                    assert (np.abs(a - b) > 1e-6).all()
    out = dn.denoise(rgb, aov, np.zeros((H, W), np.float32))
    ulp = np.abs(out.view(np.int32).astype(np.int64) - rgb.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, ulp.max()             # (c / af) * af: one rounding each way


# ---------------------------------------------------------------- quality
QUALITY_W = QUALITY_H = 64
QUALITY_SPP, REFERENCE_SPP = 16, 256


def oracle_feature_buffers(api, orc, hs, world, cam, p):
    """The feature buffer [H, W, 8] of include/hrt.h from the oracle's first hits: every sample's camera ray is the film path's own
    (orc.trace_path), its first hit the oracle's closest_hit, its albedo the attenuation of the oracle's scatter.  A sample that does not
    scatter (a light, a miss) contributes the pixel's mean one-segment radiance over such samples, clamped to [0, 1] -- the per-sample
    clamp of hrt_render_aov_* applied to their mean, which is the same value wherever a pixel's lights and sky are one colour."""
    W, H, spp = p.width, p.height, p.samples
    n = W * H
    flat = hs.flat
    medium_prim = np.array([flat.prims[i].kind == api.PRIM_MEDIUM for i in range(flat.n_prims)] or [False])
    p1 = api.Params()
    C.memmove(C.byref(p1), C.byref(p), C.sizeof(p))
    p1.max_depth = 1
    albedo, normal = np.zeros((n, 3), np.float64), np.zeros((n, 3), np.float64)
    alpha, depth, lost = np.zeros(n), np.zeros(n), np.zeros(n)
    for s in range(spp):
        rays = np.array([orc.trace_path(world, cam, p1, pidx, s, max_seg=1)[0][0] for pidx in range(n)], np.float32)
        o, d = np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:])
        _, att, flag, hits = world.scatter(p, o, d, pixel0=0)
        hit = hits["prim"] >= 0
        solid = hit & ~medium_prim[np.where(hit, hits["prim"], 0)]
        albedo += np.where((flag == 1)[:, None], att, 0.0)
        lost += flag != 1
        alpha += hit
        normal += np.where(solid[:, None], hits["normal"], 0.0)
        depth += np.where(hit, hits["t"].astype(np.float64) * np.sqrt((d.astype(np.float64) ** 2).sum(axis=1)), 0.0)
    emitted, _ = world.render_tile(cam, p1)                      # mean over all samples of what the first hit emits
    with np.errstate(all="ignore"):
        per_lost = np.clip(np.nan_to_num(emitted.reshape(n, 3) * spp / lost[:, None]), 0.0, 1.0)
    albedo += per_lost * lost[:, None]
    aov = np.concatenate([albedo / spp, (alpha / spp)[:, None], normal / spp, (depth / spp)[:, None]], axis=1)
    return aov.reshape(H, W, 8).astype(np.float32)


def quality_case(api, orc, scenes_dir, assets, scene):
    """-> (noisy film, feature buffer, reference film) of one scene"""
    hs = api.HostScene(f"{scenes_dir}/{scene}", assets)
    cam = hs.camera(QUALITY_W, QUALITY_H)
    world = orc.World(hs.flat_ptr)
    p = api.default_params(QUALITY_W, QUALITY_H, QUALITY_SPP, seed=1)
    noisy, _ = world.render_tile(cam, p)
    aov = oracle_feature_buffers(api, orc, hs, world, cam, p)
    ref, _ = world.render_tile(cam, api.default_params(QUALITY_W, QUALITY_H, REFERENCE_SPP, seed=2))
    return noisy, aov, ref


def rms(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("scene", ["cornell_box.yaml", "material_zoo.yaml"])
def test_filtering_lowers_the_rms_error_against_a_converged_film(built, assets, scenes_dir, scene):
    """64 x 64 x 16 spp oracle film, feature buffers from the oracle's first hits, default parameters, spatial variance estimate,
    against a 256 spp oracle film of another seed: the RMS error of the linear film is lower after filtering than before.
    Measured: cornell_box 0.09274 -> 0.07733 (ratio 0.834), material_zoo 0.05877 -> 0.05404 (ratio 0.920)."""
    from hobbyraytracer_amd import api
    from oracle import oracle_py as orc
    noisy, aov, ref = quality_case(api, orc, scenes_dir, assets, scene)
    assert np.isfinite(noisy).all() and np.isfinite(ref).all()
    before, after = rms(noisy, ref), rms(dn.denoise(noisy, aov), ref)
    print(f"{scene}: rms before {before:.5f}, after {after:.5f}, ratio {after / before:.4f}")
    assert after < before, (scene, before, after)
