"""The develop stage (include/hrt.h "develop") without a GPU: the C ABI is declared, exported, bound and still C99; bad
arguments are refused before any device is touched with the outputs untouched; the CLI refuses bad switches; and the numpy restatement of
the header's words (tests/develop_np.py) has the properties a bloom that conserves energy and a meter that reads stops must have.
tests/test_gpu_develop.py requires the kernels to give the restatement's bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import develop_np as dv
from tests.test_abi import ROOT, _declared_functions

DEVELOP_SYMBOLS = ("hrt_develop_defaults", "hrt_develop_workspace_bytes", "hrt_develop_device", "hrt_develop")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lit_square(side=64, square=16, value=(3.0, 2.0, 1.0)):
    """a black film with a lit centre square (tests/test_gpu_develop.py uses it too)"""
    film = np.zeros((side, side, 3), F)
    a = (side - square) // 2
    r = np.random.default_rng(3)
    film[a:a + square, a:a + square] = (np.asarray(value, F) * r.uniform(0.5, 1.5, (square, square, 1))).astype(F)
    return film


def check_lit_square(film, out, levels):
    """each channel's float64 sum within 1e-6 relative, and nothing beyond the bloom's reach: the ring outside 3 * 2^L is exactly 0"""
    side = film.shape[0]
    lit = np.argwhere(film.any(axis=-1))
    reach = 3 * 2 ** levels
    assert lit.min() >= reach and lit.max() < side - reach
    for k in range(3):
        a, b = film[..., k].astype(np.float64).sum(), out[..., k].astype(np.float64).sum()
        assert abs(a - b) <= 1e-6 * a, (k, a, b)
    ring = np.ones(film.shape[:2], bool)
    ring[lit.min() - reach:lit.max() + reach + 1, lit.min() - reach:lit.max() + reach + 1] = False
    assert ring.any() and (_bits(out[ring]) == 0).all()
    assert (out[lit.min() - 1, lit.min():lit.max()] > 0).all()            # ... while the square's rim did receive light


# ---------------------------------------------------------------- the C ABI
def test_the_symbols_are_declared_exported_and_bound(built):
    from hobbyraytracer_amd import api
    declared = _declared_functions("hrt.h")
    lib = C.CDLL(api.HIP_LIB_PATH)
    for name in DEVELOP_SYMBOLS:
        assert name in declared, f"include/hrt.h does not declare {name}"
        assert hasattr(lib, name), f"libhrt_hip.so does not export {name}"
        assert name in api.HIP_SYMBOLS
    for f in (api.develop, api.develop_device, api.develop_defaults, api.develop_workspace_bytes):
        assert callable(f)
    p = api.develop_defaults()
    assert {n: getattr(p, n) for n, _ in api.DevelopParams._fields_} == {k: (np.float32(v) if isinstance(v, float) else v) for k, v in dv.DEFAULTS.items()}
    assert api.develop_defaults(bloom_levels=3, key=0.5).bloom_levels == 3
    assert api.DEVELOP_BINS == dv.BINS == 2048
    fixed = 2048 * 4 + 32                                            # the counters and the info record's slot
    assert api.develop_workspace_bytes(640, 640, 0) == fixed
    assert api.develop_workspace_bytes(640, 640, 2) == fixed + 16 * (320 * 320 + 160 * 160)
    assert api.develop_workspace_bytes(37, 29, 8) == fixed + 16 * sum(w * h for w, h in dv.level_sizes(37, 29, 8)) and len(dv.level_sizes(37, 29, 8)) == 6
    assert api.develop_workspace_bytes(1, 1, 8) == fixed
    assert api.develop_workspace_bytes(0, 5, 1) == 0 and api.develop_workspace_bytes(1 << 16, 1 << 15, 1) == 0
    assert api.develop_workspace_bytes(8, 8, 9) == 0 and api.develop_workspace_bytes(8, 8, -1) == 0
    assert api.develop_workspace_bytes(1 << 15, 1 << 15, 1) == fixed + (16 << 28)


def test_the_header_is_c99_and_the_structs_have_the_sizes_of_their_ctypes_twins(built, tmp_path):
    from hobbyraytracer_amd import api
    src = tmp_path / "dv.c"
    src.write_text('#include <stdio.h>\n' f'#include "{ROOT}/include/hrt.h"\n'
                   "void (*a)(hrt_develop_params*) = hrt_develop_defaults;\n"
                   "uint64_t (*b)(int32_t, int32_t, int32_t) = hrt_develop_workspace_bytes;\n"
                   "hrt_status (*c)(int, int32_t, int32_t, const hrt_develop_params*, const float*, float*, hrt_develop_info*, uint32_t*, void*, void*) = "
                   "hrt_develop_device;\n"
                   "hrt_status (*d)(int, int32_t, int32_t, const hrt_develop_params*, const float*, float*, hrt_develop_info*, uint32_t*) = hrt_develop;\n"
                   'int main(void){ printf("%d %d %d\\n", (int)sizeof(hrt_develop_params), (int)sizeof(hrt_develop_info), HRT_DEVELOP_BINS); return a && b && c && d ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-o", str(tmp_path / "dv.o"), str(src)])
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "dv"), str(src), "-L" + api.LIB_DIR, "-lhrt_hip", "-Wl,-rpath," + api.LIB_DIR,
                           "-Wl,-rpath,/opt/rocm/lib"])
    sizes = [int(v) for v in subprocess.check_output([str(tmp_path / "dv")]).decode().split()]
    assert sizes == [C.sizeof(api.DevelopParams), C.sizeof(api.DevelopInfo), api.DEVELOP_BINS] == [40, 24, 2048]


def test_bad_arguments_are_refused_before_any_device_is_touched_and_leave_the_outputs_untouched(built):
    from hobbyraytracer_amd import api
    W, H = 8, 6
    rgb = np.ones((H, W, 3), np.float32)
    out = np.full((H, W, 3), 7.0, np.float32)
    hist = np.full(api.DEVELOP_BINS, 7, np.uint32)
    info = api.DevelopInfo(7.0, 7.0, 7, 7, 7)
    ws = np.zeros(api.develop_workspace_bytes(W, H, 8) // 4 + 8, np.float32)
    ws_ptr = (ws.ctypes.data + 15) & ~15
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    good = api.develop_defaults(bloom_levels=2, exposure_mode=2)

    def host(p=good, w=W, h=H, r=rgb, o=out, i=info, hi=hist):
        return api._hip.hrt_develop(0, w, h, C.byref(p) if p is not None else None, fp(r) if r is not None else None, fp(o) if o is not None else None,
                                    C.byref(i) if i is not None else None, hi.ctypes.data_as(C.POINTER(C.c_uint32)) if hi is not None else None)

    def device(p=good, w=W, h=H, r=rgb, o=out, i=info, hi=hist, s=ws_ptr):
        return api._hip.hrt_develop_device(0, w, h, C.byref(p) if p is not None else None, C.c_void_p(r.ctypes.data) if r is not None else None,
                                           C.c_void_p(o.ctypes.data) if o is not None else None, C.c_void_p(C.addressof(i)) if i is not None else None,
                                           C.c_void_p(hi.ctypes.data) if hi is not None else None, C.c_void_p(s) if s else None, None)

    def refused(st, word):
        assert st == api.HRT_ERR_INVALID, (st, word)
        assert word.encode() in api._hip.hrt_last_error(), (word, api._hip.hrt_last_error())
        assert (out == 7.0).all() and (hist == 7).all() and (rgb == 1.0).all()
        assert (info.mean_ev, info.scale, info.metered, info.levels, info.pad) == (7.0, 7.0, 7, 7, 7)

    nan, inf = float("nan"), float("inf")
    tiny = float(np.float32(2.0 ** -126)) * 0.5                 # a denormal: below the smallest floor
    bad = {"bloom_levels": (-1, 9, 100), "bloom_strength": (-0.1, 1.5, nan, inf), "exposure_mode": (-1, 3), "exposure_ev": (65.0, -64.5, nan, inf, -inf),
           "key": (0.0, -1.0, nan, inf), "meter_low": (-0.1, 0.9, 0.95, nan), "meter_high": (0.1, 0.05, 1.5, nan),
           "meter_floor": (0.0, -1.0, tiny, nan, inf), "ev_min": (17.0, nan, inf, -inf), "ev_max": (-17.0, nan, inf)}
    for call in (host, device):
        for missing in ("p", "r", "o"):
            refused(call(**{missing: None}), "NULL")
        refused(call(w=0), "width")
        refused(call(h=-3), "width")
        refused(call(w=1 << 16, h=(1 << 14) + 1), "2^30")
        for field, values in bad.items():
            for v in values:
                refused(call(p=api.develop_defaults(**{field: v})), field)
    refused(device(s=None), "NULL")
    refused(device(s=ws_ptr + 4), "misaligned")
    for odd in range(4):                                        # the film buffers and the histogram two bytes off, the info record four
        off = [(2 if k == odd else 0) for k in range(3)] + [4 if odd == 3 else 0]
        r, o, hi, i = rgb.ctypes.data + off[0], out.ctypes.data + off[1], hist.ctypes.data + off[2], C.addressof(info) + off[3]
        assert C.addressof(info) % 8 == 0
        refused(api._hip.hrt_develop(0, W, H, C.byref(good), C.cast(C.c_void_p(r), C.POINTER(C.c_float)), C.cast(C.c_void_p(o), C.POINTER(C.c_float)),
                                     C.cast(C.c_void_p(i), C.POINTER(api.DevelopInfo)), C.cast(C.c_void_p(hi), C.POINTER(C.c_uint32))), "misaligned")
        refused(api._hip.hrt_develop_device(0, W, H, C.byref(good), C.c_void_p(r), C.c_void_p(o), C.c_void_p(i), C.c_void_p(hi), C.c_void_p(ws_ptr), None),
                "misaligned")
    # the Python wrapper checks the shape and the field names itself
    with pytest.raises(ValueError):
        api.develop(rgb[:, :, :2])
    with pytest.raises(TypeError):
        api.develop_defaults(sigma=1.0)


def test_cli_usage_errors(built, tmp_path, scenes_dir):
    from hobbyraytracer_amd import api
    with open(os.path.join(scenes_dir, "cornell_box.yaml")) as f:
        (tmp_path / "s.yaml").write_text(f.read())
    for extra in (("--bloom-strength", "1.5"), ("--bloom-strength", "-0.1"), ("--bloom-strength", "nan"), ("--bloom-strength", "x"), ("--bloom-strength",),
                  ("--bloom-levels", "0"), ("--bloom-levels", "9"), ("--bloom-levels", "2.5"), ("--bloom-levels", "x"),
                  ("--exposure", "65"), ("--exposure", "-65"), ("--exposure", "nan"), ("--exposure", "inf"), ("--exposure", "bright"), ("--exposure",),
                  ("--exposure-key", "0"), ("--exposure-key", "-1"), ("--exposure-key", "nan"), ("--exposure-key", "inf"),
                  ("--exposure-window", "0.5"), ("--exposure-window", "0.5,0.5"), ("--exposure-window", "0.9,0.1"), ("--exposure-window", "-0.1,0.5"),
                  ("--exposure-window", "0.1,1.5"), ("--exposure-window", "nan,0.5"), ("--exposure-window", "0.1,0.9,1"), ("--exposure-window", "a,b"),
                  ("--exposure", "1", "--exposure-key", "0.2"), ("--exposure-key", "0.2", "--exposure", "-1"), ("--exposure-window", "0.2,0.8", "--exposure", "0"),
                  ("--dump-undeveloped", "u.pfm")):
        r = subprocess.run([api.CLI_PATH, "s.yaml", "--size", "8x8", "--spp", "1", "--no-progress", "--out", "u.png", *extra], cwd=tmp_path,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert r.stderr.strip(), extra
        assert not (tmp_path / "u.png").exists() and not (tmp_path / "u.pfm").exists()


# ---------------------------------------------------------------- properties of the restatement
def _noise(H, W, seed=1):
    r = np.random.default_rng(seed)
    return (r.uniform(0.0, 2.0, (H, W, 1)) * r.uniform(0.2, 1.0, (H, W, 3))).astype(F)


def test_a_default_struct_returns_the_bits():
    film = _noise(13, 22)
    film[3, 4] = (np.nan, 1.0, -0.0)
    film[5, 6] = (-1.0, np.inf, 2.0)
    out, m, info, hist = dv.develop(film)
    assert np.array_equal(_bits(out), _bits(film)) and info == {"mean_ev": 0.0, "scale": F(1.0), "metered": 0, "levels": 0} and not hist.any()
    for kw in ({"bloom_levels": 3, "bloom_strength": 0.0}, {"bloom_levels": 0, "bloom_strength": 1.0}):
        assert np.array_equal(_bits(dv.develop(film, **kw)[0]), _bits(film)), kw
    one = np.full((1, 1, 3), 0.25, F)                               # a 1 x 1 film has no levels
    out, _, info, _ = dv.develop(one, bloom_levels=8, bloom_strength=1.0)
    assert np.array_equal(_bits(out), _bits(one)) and info["levels"] == 0


def test_the_level_count_follows_the_larger_side():
    assert [len(dv.level_sizes(w, h, 8)) for w, h in ((1, 1), (2, 1), (2, 2), (3, 1), (16, 16), (17, 33), (37, 29), (70, 3), (257, 3))] == [0, 1, 1, 2, 4, 6, 6, 7, 8]
    assert dv.level_sizes(37, 29, 8) == [(19, 15), (10, 8), (5, 4), (3, 2), (2, 1), (1, 1)]
    assert len(dv.level_sizes(37, 29, 2)) == 2 and len(dv.level_sizes(257, 3, 8)) == 8 and dv.level_sizes(513, 1, 8)[-1] == (3, 1)


def test_a_constant_film_comes_back_bit_for_bit():
    """every weight is a dyadic fraction and each filter's weights sum to 1: on a constant 0.5 the sums are exact at every step"""
    film = np.full((29, 37, 3), 0.5, F)
    for levels in (1, 2, 3, 8):
        out, _, info, _ = dv.develop(film, bloom_levels=levels, bloom_strength=0.5)
        assert np.array_equal(_bits(out), _bits(film)), levels
        assert info["levels"] == min(levels, 6)


def test_a_lit_square_far_from_the_borders_keeps_its_sum_and_its_reach():
    film = lit_square()
    out, _, info, _ = dv.develop(film, bloom_levels=2, bloom_strength=1.0)
    assert info["levels"] == 2
    check_lit_square(film, out, 2)
    out, _, _, _ = dv.develop(film, bloom_levels=2, bloom_strength=0.25)
    check_lit_square(film, out, 2)


def test_invalid_pixels_keep_their_bits_and_add_nothing():
    film = _noise(20, 24, seed=2)
    clean = film.copy()
    payload = np.array([0x7fc01234], np.uint32).view(F)[0]
    spots = {(4, 4): (payload, 0.3, 0.2), (0, 8): (0.1, np.inf, 0.2), (19, 0): (0.1, 0.2, -np.inf)}
    for (y, x), v in spots.items():
        film[y, x] = v
        clean[y, x] = 0.0
    out, _, _, _ = dv.develop(film, bloom_levels=3, bloom_strength=0.5, exposure_mode=dv.MANUAL, exposure_ev=1.0)
    want, _, _, _ = dv.develop(clean, bloom_levels=3, bloom_strength=0.5, exposure_mode=dv.MANUAL, exposure_ev=1.0)
    ok = np.ones(film.shape[:2], bool)
    for (y, x) in spots:
        ok[y, x] = False
        assert np.array_equal(_bits(out[y, x]), _bits(film[y, x]))
    assert np.isfinite(out[ok]).all() and np.array_equal(_bits(out[ok]), _bits(want[ok]))   # as if they had been black


def test_the_bins_are_an_eighth_of_a_stop():
    def bin_of(v):
        return int(np.flatnonzero(dv.histogram(np.full((1, 1, 3), v, F), 2.0 ** -16))[0])
    # Y of a grey pixel is the grey value up to an ulp; these values sit in the middle of their bins' reach
    assert [bin_of(0.18), bin_of(1.01), bin_of(1.51)] == [995, 1016, 1020]
    l = np.array([0.18, 1.0, 1.5], F).view(np.uint32) >> 20
    assert l.tolist() == [995, 1016, 1020]
    for k in range(8):                                              # the literals of the header are the bins' middles in stops
        assert abs(dv.MID[k] - np.log2(1.0 + (k + 0.5) / 8.0)) < 1e-15


def test_doubling_a_film_moves_every_count_up_a_stop_and_halves_the_scale_exactly():
    film = _noise(31, 17, seed=4)
    film[2, 3] = 0.0
    film[5, 5] = (1e-7, 1e-7, 1e-7)                                 # below the floor in both films
    for kw in ({"exposure_mode": dv.AUTO}, {"bloom_levels": 2, "bloom_strength": 0.25, "exposure_mode": dv.AUTO}):
        _, _, a, ha = dv.develop(film, **kw)
        _, _, b, hb = dv.develop(film * F(2.0), **kw)
        assert a["metered"] == b["metered"] == (31 * 17 - 2 if "bloom_levels" not in kw else 31 * 17)   # (the bloom lights the two dark pixels)
        assert np.array_equal(hb[8:], ha[:-8]) and not hb[:8].any() and not ha[-8:].any()
        # every ev_b moves by exactly 1; the float64 sums round differently, far below an fp32 ulp of the scale
        assert abs(b["mean_ev"] - (a["mean_ev"] + 1.0)) < 1e-12 and b["scale"] * F(2.0) == a["scale"]


def test_the_default_window_meters_the_dark_level_and_ignores_the_lights():
    H, W = 20, 50
    film = np.full((H, W, 3), 0.02, F)                              # 90 % of the pixels: a dark wall, above the floor
    film[:2] = 12.0                                                 # 10 %: a light
    out, _, info, hist = dv.develop(film, exposure_mode=dv.AUTO)
    dark = int(np.array([dv.lum(F(0.02), F(0.02), F(0.02))], F).view(np.uint32)[0] >> 20)
    assert hist[dark] == 900 and hist.sum() == 1000 == info["metered"]
    ev_dark = ((dark >> 3) - 127) + dv.MID[dark & 7]
    assert abs(info["mean_ev"] - ev_dark) < 1e-12                   # the window 10 % .. 90 % lies inside the dark bin
    assert abs(float(info["scale"]) - 0.18 * 2.0 ** -ev_dark) <= 1e-6 * float(info["scale"])
    assert 0.15 < out[10, 10, 0] < 0.22                             # the wall lands near the key (to within its bin, an eighth of a stop)
    # the clamp
    _, _, clamped, _ = dv.develop(film, exposure_mode=dv.AUTO, ev_min=-2.0)
    assert clamped["mean_ev"] == -2.0 and clamped["scale"] == F(0.18 * 4.0)


def test_a_film_with_no_metered_pixel_gives_scale_1():
    film = np.zeros((5, 7, 3), F)
    film[0, 0] = np.nan
    film[1, 1] = (-3.0, -2.0, -1.0)
    film[2, 2] = (1e-6, 1e-6, 1e-6)                                 # below the floor of 2^-16
    out, _, info, hist = dv.develop(film, exposure_mode=dv.AUTO)
    assert info == {"mean_ev": 0.0, "scale": F(1.0), "metered": 0, "levels": 0} and not hist.any()
    assert np.array_equal(_bits(out), _bits(film))


def test_the_golden_films_auto_scales_are_printed_not_asserted():
    """The table of DESIGN.md 4.17: the committed scenes sit 45 x apart."""
    films = np.load(os.path.join(ROOT, "tests", "golden", "films.npz"))
    for name in ("cornell_box_ref", "teapot_scene_ref", "material_zoo_ref", "three_meshes_ref"):
        if name in films.files:
            _, _, info, _ = dv.develop(films[name], exposure_mode=dv.AUTO)
            print(f"{name}: {films[name].shape[1]} x {films[name].shape[0]}, metered {info['metered']}, mean_ev {info['mean_ev']:.3f}, scale {float(info['scale']):.4g}")
