"""The outlier filter (include/hrt.h "despeckle") without a GPU: the C ABI is declared, exported, bound and still C99; bad
arguments are refused before any device is touched with the outputs untouched; the CLI refuses bad switches; the numpy restatement of the
header's words (tests/despeckle_np.py) has the properties an energy-preserving outlier filter must have; and it lowers the error of a
noisy oracle film against a converged one, alone and ahead of the denoiser -- the quality test, decided here because GPU films are the
oracle's bits (tests/test_gpu_despeckle.py requires the kernels to give the restatement's bits)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import denoise_np as dn
from tests import despeckle_np as ds
from tests.test_abi import ROOT, _declared_functions

DESPECKLE_SYMBOLS = ("hrt_despeckle_defaults", "hrt_despeckle_workspace_bytes", "hrt_despeckle_device", "hrt_despeckle")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the C ABI
def test_the_symbols_are_declared_exported_and_bound(built):
    from hobbyraytracer_amd import api
    declared = _declared_functions("hrt.h")
    lib = C.CDLL(api.HIP_LIB_PATH)
    for name in DESPECKLE_SYMBOLS:
        assert name in declared, f"include/hrt.h does not declare {name}"
        assert hasattr(lib, name), f"libhrt_hip.so does not export {name}"
        assert name in api.HIP_SYMBOLS
    for f in (api.despeckle, api.despeckle_device, api.despeckle_defaults, api.despeckle_workspace_bytes):
        assert callable(f)
    p = api.despeckle_defaults()
    assert {n: getattr(p, n) for n, _ in api.DespeckleParams._fields_} == {k: (np.float32(v) if isinstance(v, float) else v) for k, v in ds.DEFAULTS.items()}
    assert api.despeckle_defaults(rank=3, ratio=1.5).rank == 3
    assert api.despeckle_workspace_bytes(640, 640) == 20 * 640 * 640
    assert api.despeckle_workspace_bytes(0, 5) == 0 and api.despeckle_workspace_bytes(1 << 16, 1 << 15) == 0 and api.despeckle_workspace_bytes(1 << 15, 1 << 15) == 20 << 30


def test_the_header_is_c99_and_the_params_struct_has_the_size_of_its_ctypes_twin(built, tmp_path):
    from hobbyraytracer_amd import api
    src = tmp_path / "ds.c"
    src.write_text('#include <stdio.h>\n' f'#include "{ROOT}/include/hrt.h"\n'
                   "void (*a)(hrt_despeckle_params*) = hrt_despeckle_defaults;\n"
                   "uint64_t (*b)(int32_t, int32_t) = hrt_despeckle_workspace_bytes;\n"
                   "hrt_status (*c)(int, int32_t, int32_t, const hrt_despeckle_params*, const float*, const float*, float*, float*, void*, void*) = "
                   "hrt_despeckle_device;\n"
                   "hrt_status (*d)(int, int32_t, int32_t, const hrt_despeckle_params*, const float*, const float*, float*, float*) = hrt_despeckle;\n"
                   'int main(void){ printf("%d\\n", (int)sizeof(hrt_despeckle_params)); return a && b && c && d ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-o", str(tmp_path / "ds.o"), str(src)])
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "ds"), str(src), "-L" + api.LIB_DIR, "-lhrt_hip", "-Wl,-rpath," + api.LIB_DIR,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert int(subprocess.check_output([str(tmp_path / "ds")]).decode()) == C.sizeof(api.DespeckleParams) == 20


def test_bad_arguments_are_refused_before_any_device_is_touched_and_leave_the_outputs_untouched(built):
    from hobbyraytracer_amd import api
    W, H = 8, 6
    rgb, var = np.ones((H, W, 3), np.float32), np.ones((H, W), np.float32)
    out, dmap = np.full((H, W, 3), 7.0, np.float32), np.full((H, W), 7.0, np.float32)
    ws = np.zeros(api.despeckle_workspace_bytes(W, H) // 4 + 8, np.float32)
    ws_ptr = (ws.ctypes.data + 15) & ~15
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    vp = lambda a: C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a)      # noqa: E731
    good = api.despeckle_defaults()

    def host(p=good, w=W, h=H, r=rgb, v=var, o=out, m=dmap):
        return api._hip.hrt_despeckle(0, w, h, C.byref(p) if p is not None else None, fp(r) if r is not None else None,
                                      fp(v) if v is not None else None, fp(o) if o is not None else None, fp(m) if m is not None else None)

    def device(p=good, w=W, h=H, r=rgb, v=var, o=out, m=dmap, s=ws_ptr):
        return api._hip.hrt_despeckle_device(0, w, h, C.byref(p) if p is not None else None, vp(r) if r is not None else None,
                                             vp(v) if v is not None else None, vp(o) if o is not None else None, vp(m) if m is not None else None,
                                             C.c_void_p(s) if s else None, None)

    def refused(st, word):
        assert st == api.HRT_ERR_INVALID, (st, word)
        assert word.encode() in api._hip.hrt_last_error(), (word, api._hip.hrt_last_error())
        assert (out == 7.0).all() and (dmap == 7.0).all() and (rgb == 1.0).all()

    for call in (host, device):
        for missing in ("p", "r", "o"):
            refused(call(**{missing: None}), "NULL")
        refused(call(w=0), "width")
        refused(call(h=-3), "width")
        refused(call(w=1 << 16, h=(1 << 14) + 1), "2^30")
        bad = {"radius": (0, 3, -1), "rank": (0, 5, -2), "ratio": (1.0, 0.5, -3.0, float("nan"), float("inf")),
               "gate_z": (-0.5, float("nan"), float("inf")), "repair_invalid": (2, -1)}
        for field, values in bad.items():
            for v in values:
                refused(call(p=api.despeckle_defaults(**{field: v})), field)
        refused(call(o=rgb), "out == rgb")
    refused(device(s=None), "NULL")
    refused(device(s=ws_ptr + 4), "misaligned")
    buffers = (rgb, var, out, dmap)
    for odd in range(4):                                       # each float buffer in turn, two bytes off
        ptrs = [a.ctypes.data + (2 if k == odd else 0) for k, a in enumerate(buffers)]
        refused(api._hip.hrt_despeckle(0, W, H, C.byref(good), *[C.cast(C.c_void_p(q), C.POINTER(C.c_float)) for q in ptrs]), "misaligned")
        refused(api._hip.hrt_despeckle_device(0, W, H, C.byref(good), *[C.c_void_p(q) for q in ptrs], C.c_void_p(ws_ptr), None), "misaligned")
    # the Python wrapper checks the shapes itself
    with pytest.raises(ValueError):
        api.despeckle(rgb[:, :, :2])
    with pytest.raises(ValueError):
        api.despeckle(rgb, variance=var[:, :4])
    with pytest.raises(TypeError):
        api.despeckle_defaults(sigma=1.0)


def test_cli_usage_errors(built, tmp_path, scenes_dir):
    from hobbyraytracer_amd import api
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    for extra in (("--despeckle-ratio", "1"), ("--despeckle-ratio", "0.5"), ("--despeckle-ratio", "nan"), ("--despeckle-ratio", "inf"),
                  ("--despeckle-ratio", "x"), ("--despeckle-rank", "0"), ("--despeckle-rank", "5"), ("--despeckle-rank", "2.5"),
                  ("--despeckle-radius", "0"), ("--despeckle-radius", "3"), ("--despeckle-gate", "-1"), ("--despeckle-gate", "nan"),
                  ("--despeckle-gate", "inf"), ("--despeckle-map", "u.pfm"), ("--despeckle-ratio",), ("--dump-noisy", "u.pfm")):
        r = subprocess.run([api.CLI_PATH, "s.yaml", "--size", "8x8", "--spp", "1", "--no-progress", "--out", "u.png", *extra], cwd=tmp_path,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "u.png").exists() and not (tmp_path / "u.pfm").exists()


# ---------------------------------------------------------------- properties of the restatement
def _ramp(H, W):
    """a smooth film whose neighbouring pixels differ by far less than the factor `ratio`"""
    y, x = np.mgrid[0:H, 0:W]
    base = (1.0 + 0.05 * x + 0.03 * y).astype(F)
    return np.stack([base * F(0.9), base * F(0.6), base * F(0.3)], axis=-1).astype(F)


def test_a_film_without_outliers_comes_back_bit_for_bit():
    H, W = 13, 22
    flat = np.empty((H, W, 3), F)
    flat[...] = (0.37, 1.9, 0.052)
    for film in (flat, _ramp(H, W)):
        for kw in ({}, {"radius": 2, "rank": 4}, {"rank": 1, "ratio": 1.5}):
            for var in (None, np.full((H, W), 0.01, F)):
                out, m = ds.despeckle(film, var, **kw)
                assert np.array_equal(_bits(out), _bits(film)), kw
                assert (m == 0).all()


@pytest.mark.parametrize("where", ["interior", "edge", "corner"])
@pytest.mark.parametrize("radius", [1, 2])
def test_a_planted_spike_is_brought_to_its_yardstick_and_every_channels_sum_is_kept(where, radius):
    H, W = 15, 18
    film = _ramp(H, W)
    y, x = {"interior": (7, 9), "edge": (0, 6), "corner": (H - 1, W - 1)}[where]
    l = ds.lum(film[..., 0], film[..., 1], film[..., 2])
    win = l[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1].ravel().tolist()
    win.remove(l[y, x])
    ref = sorted(win)[-2]                                       # the second-largest neighbour: the default rank
    film[y, x] = film[y, x] * F(ref * 50 / l[y, x])
    out, m = ds.despeckle(film, radius=radius)
    lo = ds.lum(out[..., 0], out[..., 1], out[..., 2])
    n = len(win) + 1
    # its kept part is the yardstick (two roundings), and it gets one share of its own excess back
    want = ref + (ds.lum(*film[y, x]) - ref) / n
    assert abs(lo[y, x] - want) <= 1e-5 * want, (lo[y, x], want)
    assert abs(float(m[y, x]) - (1.0 - 1.0 / 50.0)) < 1e-5 and np.count_nonzero(m) == 1
    for k in range(3):
        a, b = film[..., k].astype(np.float64).sum(), out[..., k].astype(np.float64).sum()
        assert abs(a - b) <= 1e-5 * a, (k, a, b)
    far = np.ones((H, W), bool)
    far[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1] = False
    assert np.array_equal(_bits(out[far]), _bits(film[far]))     # nothing outside the spike's window moved
    near = ~far
    near[y, x] = False
    assert (out[near] > film[near]).all()                        # ... and every neighbour gained


def test_two_adjacent_spikes_fall_with_rank_2_and_stand_with_rank_1():
    film = _ramp(12, 12)
    before = film.copy()
    film[5, 5] *= F(40)
    film[5, 6] *= F(60)
    out, m = ds.despeckle(film, rank=2)
    assert m[5, 5] > 0.9 and m[5, 6] > 0.9 and np.count_nonzero(m) == 2
    l_out, l_in = ds.lum(*np.moveaxis(out, -1, 0)), ds.lum(*np.moveaxis(before, -1, 0))
    assert l_out[5, 5] < 20 * l_in[5, 5] and l_out[5, 6] < 20 * l_in[5, 6]
    out1, m1 = ds.despeckle(film, rank=1)
    assert (m1 == 0).all() and np.array_equal(_bits(out1), _bits(film))


def test_a_one_pixel_wide_bright_line_is_untouched_with_rank_2():
    """Every pixel of a line has two neighbours as bright as itself, so the second-largest neighbour is no yardstick to fall to.  The line
    here is closed (the outline of a rectangle); of an open line, the same holds for every pixel but its two ends, which have one bright
    neighbour each and are, by the definition, outliers of rank 2 -- asserted too, so that nobody takes it for a bug."""
    film = _ramp(12, 14)
    ring = np.zeros((12, 14), bool)
    ring[2:9, 3:11] = True
    ring[3:8, 4:10] = False
    film[ring] *= F(30)
    for radius in (1, 2):
        out, m = ds.despeckle(film, rank=2, radius=radius)
        assert (m == 0).all() and np.array_equal(_bits(out), _bits(film))
    open_line = _ramp(12, 14)
    open_line[:, 6] *= F(30)
    _, m = ds.despeckle(open_line, rank=2)
    assert (m[1:-1] == 0).all() and np.count_nonzero(m) == 2 and m[0, 6] > 0 and m[-1, 6] > 0


def test_the_variance_gate_spares_a_highlight_and_lets_a_spike_through():
    film = _ramp(11, 11)
    film[4, 7] *= F(50)
    _, m_free = ds.despeckle(film)
    assert m_free[4, 7] > 0
    l = ds.lum(*np.moveaxis(film, -1, 0))
    ref = np.sort(np.delete(l[3:6, 6:9].ravel(), 4))[-2]
    excess = l[4, 7] - ref
    out, m = ds.despeckle(film, np.zeros((11, 11), F), gate_z=2.0)
    assert (m == 0).all() and np.array_equal(_bits(out), _bits(film))            # no variance: a real highlight
    out, m = ds.despeckle(film, np.full((11, 11), excess * excess, F), gate_z=2.0)
    assert m[4, 7] > 0 and np.count_nonzero(m) == 1                              # a standard deviation of the excess: a spike
    out, m = ds.despeckle(film, np.zeros((11, 11), F), gate_z=0.0)
    assert m[4, 7] > 0                                                           # gate_z 0: no gate
    for v in (-1.0, np.nan):                                                     # counted as 0
        assert (ds.despeckle(film, np.full((11, 11), v, F))[1] == 0).all()


def test_invalid_pixels_are_repaired_to_their_neighbours_mean_and_move_no_neighbour():
    H, W = 9, 10
    film = _ramp(H, W)
    bad = film.copy()
    payload = np.array([0x7fc01234], np.uint32).view(F)[0]
    spots = {(4, 4): (payload, 0.3, 0.2), (0, 8): (0.1, np.inf, 0.2), (H - 1, 0): (0.1, 0.2, -np.inf)}
    for (y, x), v in spots.items():
        bad[y, x] = v
    out, m = ds.despeckle(bad)
    ok = np.ones((H, W), bool)
    for (y, x) in spots:
        ok[y, x] = False
        win = film[max(0, y - 1):y + 2, max(0, x - 1):x + 2].reshape(-1, 3).astype(np.float64)
        mean = (win.sum(axis=0) - film[y, x]) / (len(win) - 1)
        assert np.allclose(out[y, x], mean, rtol=1e-6, atol=0), (y, x)
        assert m[y, x] == -1
    assert np.array_equal(_bits(out[ok]), _bits(film[ok])) and (m[ok] == 0).all()
    out, m = ds.despeckle(bad, repair_invalid=0)
    assert np.array_equal(_bits(out), _bits(bad)) and (m == 0).all()
    one = np.full((1, 1, 3), np.nan, F)
    out, m = ds.despeckle(one)
    assert np.array_equal(_bits(out), _bits(one)) and m[0, 0] == 0
    # an invalid pixel is never counted: a spike beside one deals its excess over the valid pixels only
    film2 = _ramp(H, W)
    film2[4, 5] *= F(50)
    film2[4, 4] = np.nan
    out, m = ds.despeckle(film2, repair_invalid=0)
    assert m[4, 5] > 0 and np.isnan(out[4, 4]).all()
    valid = np.isfinite(film2).all(axis=-1)
    for k in range(3):
        a, b = film2[..., k][valid].astype(np.float64).sum(), out[..., k][valid].astype(np.float64).sum()
        assert abs(a - b) <= 1e-5 * a


# ---------------------------------------------------------------- quality
@pytest.fixture(scope="module")
def cases(built, assets, scenes_dir):
    from hobbyraytracer_amd import api
    from oracle import oracle_py as orc
    from tests.test_denoise_cpu import QUALITY_H, QUALITY_SPP, QUALITY_W, REFERENCE_SPP, oracle_feature_buffers
    cache = {}

    def get(scene, with_aov=False):
        if scene not in cache:
            hs = api.HostScene(f"{scenes_dir}/{scene}", assets)
            cam = hs.camera(QUALITY_W, QUALITY_H)
            world = orc.World(hs.flat_ptr)
            p = api.default_params(QUALITY_W, QUALITY_H, QUALITY_SPP, seed=1)
            noisy, _ = world.render_tile(cam, p)
            ref, _ = world.render_tile(cam, api.default_params(QUALITY_W, QUALITY_H, REFERENCE_SPP, seed=2))
            cache[scene] = [noisy, ref, None, (hs, world, cam, p)]
        if with_aov and cache[scene][2] is None:
            hs, world, cam, p = cache[scene][3]
            cache[scene][2] = oracle_feature_buffers(api, orc, hs, world, cam, p)
        return cache[scene][:3]
    return get


def _rms(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("scene", ["cornell_box.yaml", "teapot_scene.yaml"])
def test_despeckling_lowers_the_rms_error_against_a_converged_film(cases, scene):
    """64 x 64 x 16 spp oracle film (the recipe of tests/test_denoise_cpu.py's quality_case), default parameters, no variance, against a
    256 spp oracle film of another seed: the RMS error of the linear film is lower after the pass than before.  Measured (DESIGN.md
    4.15): cornell_box ratio 0.905, teapot_scene 0.758."""
    noisy, ref, _ = cases(scene)
    assert np.isfinite(noisy).all() and np.isfinite(ref).all()
    out, m = ds.despeckle(noisy)
    before, after = _rms(noisy, ref), _rms(out, ref)
    print(f"{scene}: rms before {before:.5f}, after {after:.5f}, ratio {after / before:.4f}, outliers {int((m > 0).sum())}")
    assert after < before, (scene, before, after)


def test_despeckling_ahead_of_the_denoiser_beats_the_denoiser_alone(cases):
    """cornell_box, the same films: despeckle and then tests/denoise_np.py's denoiser (spatial variance estimate) has a lower RMS error
    than the denoiser alone.  Measured: 0.760 against 0.834 of the noisy film's error."""
    noisy, ref, aov = cases("cornell_box.yaml", with_aov=True)
    before = _rms(noisy, ref)
    alone = _rms(dn.denoise(noisy, aov), ref)
    both = _rms(dn.denoise(ds.despeckle(noisy)[0], aov), ref)
    print(f"cornell_box.yaml: denoiser alone {alone / before:.4f}, despeckle then denoiser {both / before:.4f} of the noisy film's rms error {before:.5f}")
    assert both < alone, (both, alone)


def test_material_zoo_is_printed_not_asserted(cases):
    """The scene the pass does not help: its film is smooth and only a handful of pixels are touched."""
    noisy, ref, _ = cases("material_zoo.yaml")
    out, m = ds.despeckle(noisy)
    print(f"material_zoo.yaml: ratio {_rms(out, ref) / _rms(noisy, ref):.4f}, outliers {int((m > 0).sum())}")
