"""The C ABI of the feature buffers without a GPU: the three hrt_render_aov_* entry points are declared in
include/hrt.h, exported by libhrt_hip.so and bound by hobbyraytracer_amd/api.py; the header is still C99; and no existing ABI struct
changed its size (tests/test_abi.py's method: sizeof from a C compiler against the ctypes mirrors).  Refusals that need no device are
checked here too; the rest of them in tests/test_gpu_aov.py."""
import ctypes as C
import subprocess

import numpy as np

from tests.test_abi import ROOT, _declared_functions

AOV_SYMBOLS = ("hrt_render_aov_tile", "hrt_render_aov_stripes_device", "hrt_render_aov_stripes")


def test_the_three_symbols_are_declared_exported_and_bound(built):
    from hobbyraytracer_amd import api
    declared = _declared_functions("hrt.h")
    lib = C.CDLL(api.HIP_LIB_PATH)
    for name in AOV_SYMBOLS:
        assert name in declared, f"include/hrt.h does not declare {name}"
        assert hasattr(lib, name), f"libhrt_hip.so does not export {name}"
        assert name in api.HIP_SYMBOLS
    for method in ("render_aov_tile", "render_aov_stripes", "render_aov_stripes_device"):
        assert callable(getattr(api.DeviceScene, method))
    assert callable(api.split_aov)


def test_the_header_is_still_c99_and_declares_the_documented_signatures(built, tmp_path):
    src = tmp_path / "aov.c"
    src.write_text(f'#include "{ROOT}/include/hrt.h"\n'
                   "hrt_status (*a)(hrt_scene*, const hrt_camera*, const hrt_params*, hrt_rect, float*) = hrt_render_aov_tile;\n"
                   "hrt_status (*b)(hrt_scene*, const hrt_camera*, const hrt_params*, int32_t, int32_t, int32_t, float*, int32_t, int32_t, void*) = "
                   "hrt_render_aov_stripes_device;\n"
                   "hrt_status (*c)(hrt_scene*, const hrt_camera*, const hrt_params*, int32_t, int32_t, int32_t, float*, int32_t, int32_t) = "
                   "hrt_render_aov_stripes;\n"
                   "int main(void){ return a && b && c ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-o", str(tmp_path / "aov.o"), str(src)])


def test_no_abi_struct_changed_its_size(built, tmp_path):
    from hobbyraytracer_amd import api
    structs = {"hrt_xform": api.Xform, "hrt_prim": api.Prim, "hrt_matvec3": api.MatVec3, "hrt_matscalar": api.MatScalar,
               "hrt_material": api.Material, "hrt_texture": api.Texture, "hrt_mesh": api.Mesh, "hrt_bvh_node": api.BvhNode,
               "hrt_flat_scene": api.FlatScene, "hrt_camera": api.Camera, "hrt_params": api.Params, "hrt_rect": api.Rect,
               "hrt_stats": api.Stats, "hrt_hit": api.Hit, "hrt_adaptive": api.Adaptive}
    # the sizes before the feature buffers: none of them may move
    before = {"hrt_xform": 20, "hrt_prim": 140, "hrt_matvec3": 16, "hrt_matscalar": 8, "hrt_material": 40, "hrt_texture": 48,
              "hrt_mesh": 16, "hrt_bvh_node": 64, "hrt_flat_scene": 168, "hrt_camera": 76, "hrt_params": 36, "hrt_rect": 16,
              "hrt_stats": 104, "hrt_hit": 48, "hrt_adaptive": 16}
    src = tmp_path / "sz.c"
    lines = ['#include <stdio.h>', f'#include "{ROOT}/include/hrt.h"', 'int main(void){']
    lines += [f'printf("{n} %zu\\n", sizeof({n}));' for n in structs]
    lines += ['return 0;}']
    src.write_text("\n".join(lines))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for n, t in structs.items():
        assert int(out[n]) == C.sizeof(t) == before[n], (n, out[n], C.sizeof(t), before[n])


def test_split_aov_names_the_eight_channels():
    from hobbyraytracer_amd import api
    buf = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    d = api.split_aov(buf)
    assert d["albedo"].shape == (2, 3, 3) and d["alpha"].shape == (2, 3) and d["normal"].shape == (2, 3, 3) and d["depth"].shape == (2, 3)
    assert np.array_equal(d["albedo"][1, 2], buf[1, 2, 0:3]) and d["alpha"][1, 2] == buf[1, 2, 3]
    assert np.array_equal(d["normal"][1, 2], buf[1, 2, 4:7]) and d["depth"][1, 2] == buf[1, 2, 7]


def test_null_arguments_are_refused_before_any_device_is_touched(built):
    from hobbyraytracer_amd import api
    cam, p = api.Camera(), api.default_params(8, 8, 1)
    out = np.full(8 * 8 * 8, 7.0, np.float32)
    ptr = out.ctypes.data_as(C.POINTER(C.c_float))
    assert api._hip.hrt_render_aov_tile(None, C.byref(cam), C.byref(p), api.Rect(0, 0, 8, 8), ptr) == api.HRT_ERR_INVALID
    assert b"NULL" in api._hip.hrt_last_error()
    assert api._hip.hrt_render_aov_stripes(None, C.byref(cam), C.byref(p), 4, 0, 1, ptr, 0, -1) == api.HRT_ERR_INVALID
    assert api._hip.hrt_render_aov_stripes_device(None, C.byref(cam), C.byref(p), 4, 0, 1, C.c_void_p(out.ctypes.data), 0, -1, None) == api.HRT_ERR_INVALID
    assert (out == 7.0).all()
