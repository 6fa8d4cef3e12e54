"""ctypes bindings of include/hrt.h (libhrt_hip.so) and include/hrt_host.h (libhrt_host.so).

Struct layouts mirror the headers field for field; ``tests/test_abi.py`` checks the sizes
against ``sizeof`` values compiled from the headers.  Every wrapper raises :class:`HrtError`
on a non-zero ``hrt_status`` — nothing here falls back to a CPU path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
HIP_LIB_PATH = os.environ.get("HRT_HIP_LIB") or os.path.join(LIB_DIR, "libhrt_hip.so")   # HRT_HIP_LIB: an instrumented build of the
# same library (-DHRT_DEBUG_BOUNDS, profiling variants; tests/tools), never another implementation
HOST_LIB_PATH = os.path.join(LIB_DIR, "libhrt_host.so")
CLI_PATH = os.path.join(_HERE, "bin", "hobbyraytracer")


class HrtError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"hrt status {status}: {message}")
        self.status = status


# ---------------------------------------------------------------- constants (hrt.h)
HRT_OK, HRT_ERR_INVALID, HRT_ERR_HIP, HRT_ERR_NO_DEVICE, HRT_ERR_OOM, HRT_ERR_IO, HRT_ERR_PARSE, HRT_ERR_UNSUPPORTED = range(8)
PRIM_SPHERE, PRIM_XY_RECT, PRIM_XZ_RECT, PRIM_YZ_RECT, PRIM_BOX, PRIM_MESH, PRIM_MEDIUM, PRIM_TRIANGLE = range(8)
XF_TRANSLATE, XF_SCALE, XF_ROTATE_QUAT, XF_ROTATE_Y = range(4)
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_ISOTROPIC, MAT_PBR, MAT_UVTEST = range(7)
TEX_SOLID, TEX_CHECKER, TEX_IMAGE, TEX_ENV = range(4)
MAX_XFORMS = 4
Q1_ROTQ_NORMALIZE, Q2_TRI_NO_TMIN, Q3_TRI_NO_FACE, Q4_SHEAR_FROM_ORIGIN = 1, 2, 4, 8
QUIRKS_REFERENCE, QUIRKS_FIXED = 0xF, 0x0
FLAG_STATS, FLAG_MEGAKERNEL, FLAG_TIMING, FLAG_THIN_LENS, FLAG_PROGRESS, FLAG_NEE, FLAG_NEE_ENV = 1, 2, 4, 8, 16, 32, 64
FLAG_NEE_EMITTERS = 128
FLAG_NEE_LOBES = 256
FLAG_STRATIFIED = 512
FLAG_ROULETTE = 1024
ROULETTE_FIRST_BOUNCE, ROULETTE_Q_FLOOR = 3, 0.05   # what a new scene has (hrt_scene_set_roulette)
FLAG_FILTER = 2048
FILTER_TENT, FILTER_BSPLINE, FILTER_MITCHELL = 0, 1, 2
FILTER_KINDS = {"tent": FILTER_TENT, "bspline": FILTER_BSPLINE, "mitchell": FILTER_MITCHELL}
FILTER_DEFAULT_RADIUS = {FILTER_TENT: 1.0, FILTER_BSPLINE: 2.0, FILTER_MITCHELL: 2.0}   # a new scene has Mitchell at 2 (hrt_scene_set_filter)


# ---------------------------------------------------------------- structs (hrt.h)
class Xform(C.Structure):
    _fields_ = [("kind", C.c_int32), ("v", C.c_float * 4)]


class Prim(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("mesh", C.c_int32), ("boundary_kind", C.c_int32),
                ("p", C.c_float * 9), ("density", C.c_float), ("n_xforms", C.c_int32), ("xf", Xform * MAX_XFORMS)]


class MatVec3(C.Structure):
    _fields_ = [("tex", C.c_int32), ("c", C.c_float * 3)]


class MatScalar(C.Structure):
    _fields_ = [("tex", C.c_int32), ("c", C.c_float)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("albedo", MatVec3), ("s0", MatScalar), ("s1", MatScalar), ("mix_tex", C.c_int32)]


class Texture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("c", C.c_float * 3), ("even", C.c_int32), ("odd", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("channels", C.c_int32), ("_pad", C.c_int32), ("offset", C.c_uint64)]


class Mesh(C.Structure):
    _fields_ = [("tri_first", C.c_uint32), ("tri_count", C.c_uint32), ("node_first", C.c_uint32), ("node_count", C.c_uint32)]


class BvhNode(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("c0_min_x", "c0_max_x", "c0_min_y", "c0_max_y", "c1_min_x", "c1_max_x", "c1_min_y",
                                         "c1_max_y", "c0_min_z", "c0_max_z", "c1_min_z", "c1_max_z")] + \
               [("child0", C.c_int32), ("child1", C.c_int32), ("_pad0", C.c_int32), ("_pad1", C.c_int32)]


class FlatScene(C.Structure):
    _fields_ = [("n_prims", C.c_uint32), ("prims", C.POINTER(Prim)),
                ("n_materials", C.c_uint32), ("materials", C.POINTER(Material)),
                ("n_textures", C.c_uint32), ("textures", C.POINTER(Texture)),
                ("n_meshes", C.c_uint32), ("meshes", C.POINTER(Mesh)),
                ("n_tris", C.c_uint64), ("tri_pos", C.POINTER(C.c_float)), ("tri_nrm", C.POINTER(C.c_float)),
                ("tri_uv", C.POINTER(C.c_float)), ("tri_box", C.POINTER(C.c_float)), ("tri_ref_order", C.POINTER(C.c_uint32)),
                ("n_nodes", C.c_uint64), ("nodes", C.POINTER(BvhNode)),
                ("n_texels_u8", C.c_uint64), ("texels_u8", C.POINTER(C.c_uint8)),
                ("n_texels_f32", C.c_uint64), ("texels_f32", C.POINTER(C.c_float)),
                ("background_tex", C.c_int32), ("_pad", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lower_left", C.c_float * 3), ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3),
                ("lens_u", C.c_float * 3), ("lens_v", C.c_float * 3), ("lens_radius", C.c_float)]


class Params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("max_depth", C.c_int32),
                ("t_min", C.c_float), ("quirks", C.c_uint32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("flags", C.c_uint32)]


class Rect(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("samples", C.c_uint64), ("box_tests", C.c_uint64), ("tri_tests", C.c_uint64),
                ("mesh_hits", C.c_uint64), ("env_lookups", C.c_uint64), ("kernel_ms", C.c_double), ("launches", C.c_uint64),
                ("traversal_ms", C.c_double), ("traversal_launches", C.c_uint64),
                ("traversal_box_tests", C.c_uint64), ("traversal_tri_tests", C.c_uint64), ("shadow_rays", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}

    def algorithmic_bytes(self, n_pixels=0):
        """32 B per box tested, 36 B per triangle tested, 60 B of attributes per
        mesh hit, 12 B per fp32 environment lookup, 12 B per pixel written."""
        return 32 * self.box_tests + 36 * self.tri_tests + 60 * self.mesh_hits + 12 * self.env_lookups + 12 * n_pixels


class Adaptive(C.Structure):
    """hrt_adaptive: the schedule and stopping rule of an adaptive render (include/hrt.h)."""
    _fields_ = [("min_samples", C.c_int32), ("pass_samples", C.c_int32), ("threshold", C.c_float), ("floor", C.c_float)]


class DenoiseParams(C.Structure):
    """hrt_denoise_params: the guided denoiser's settings (include/hrt.h); denoise_defaults() fills them in."""
    _fields_ = [("iterations", C.c_int32), ("normal_squarings", C.c_int32), ("sigma_l", C.c_float), ("sigma_z", C.c_float),
                ("albedo_floor", C.c_float)]


class DespeckleParams(C.Structure):
    """hrt_despeckle_params: the outlier filter's settings (include/hrt.h); despeckle_defaults() fills them in."""
    _fields_ = [("radius", C.c_int32), ("rank", C.c_int32), ("ratio", C.c_float), ("gate_z", C.c_float), ("repair_invalid", C.c_int32)]


class DevelopParams(C.Structure):
    """hrt_develop_params: the develop stage's settings (include/hrt.h); develop_defaults() fills them in."""
    _fields_ = [("bloom_levels", C.c_int32), ("bloom_strength", C.c_float), ("exposure_mode", C.c_int32), ("exposure_ev", C.c_float),
                ("key", C.c_float), ("meter_low", C.c_float), ("meter_high", C.c_float), ("meter_floor", C.c_float), ("ev_min", C.c_float),
                ("ev_max", C.c_float)]


class DevelopInfo(C.Structure):
    """hrt_develop_info: what a develop call measured and applied (include/hrt.h)."""
    _fields_ = [("mean_ev", C.c_double), ("scale", C.c_float), ("metered", C.c_uint32), ("levels", C.c_uint32), ("pad", C.c_uint32)]


DEVELOP_BINS = 2048
EXPOSURE_NONE, EXPOSURE_MANUAL, EXPOSURE_AUTO = 0, 1, 2


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("prim", C.c_int32), ("tri", C.c_int32), ("front_face", C.c_int32), ("p", C.c_float * 3),
                ("normal", C.c_float * 3), ("u", C.c_float), ("v", C.c_float)]


HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4"), ("tri", "<i4"), ("front_face", "<i4"), ("p", "<f4", 3),
                      ("normal", "<f4", 3), ("u", "<f4"), ("v", "<f4")])
assert HIT_DTYPE.itemsize == C.sizeof(Hit)

HIP_SYMBOLS = ["hrt_device_count", "hrt_scene_create", "hrt_scene_destroy", "hrt_render_tile", "hrt_render_stripes_device",
               "hrt_render_stripes", "hrt_render_stripes_accumulate_device", "hrt_render_stripes_accumulate", "hrt_stripe_rows", "hrt_stripe_row_index", "hrt_scene_stats", "hrt_resolve_u8",
               "hrt_resolve_u8_device", "hrt_closest_hit", "hrt_math_probe", "hrt_sampler_probe", "hrt_status_str", "hrt_last_error", "hrt_version",
               "hrt_multi_create", "hrt_multi_destroy", "hrt_multi_devices", "hrt_multi_uses_rccl", "hrt_multi_render", "hrt_bvh_build_device", "hrt_bvh_build_sah",
               "hrt_debug_bounds_violations", "hrt_scene_progress", "hrt_multi_progress",
               "hrt_render_stripes_adaptive_device", "hrt_render_stripes_adaptive", "hrt_adaptive_mean_device", "hrt_env_table_build",
               "hrt_emitter_table_build", "hrt_scene_set_roulette", "hrt_multi_set_roulette",
               "hrt_render_aov_tile", "hrt_render_aov_stripes_device", "hrt_render_aov_stripes",
               "hrt_aov_ids_bytes", "hrt_render_aov_ids_tile", "hrt_render_aov_ids_stripes_device", "hrt_render_aov_ids_stripes",
               "hrt_denoise_defaults", "hrt_denoise_workspace_bytes", "hrt_denoise_device", "hrt_denoise", "hrt_denoise_resolve_u8",
               "hrt_variance_state_bytes", "hrt_variance_fold_device", "hrt_variance_finish_device", "hrt_adaptive_variance_device",
               "hrt_variance_fold", "hrt_variance_finish", "hrt_adaptive_variance",
               "hrt_despeckle_defaults", "hrt_despeckle_workspace_bytes", "hrt_despeckle_device", "hrt_despeckle",
               "hrt_scene_set_filter", "hrt_multi_set_filter", "hrt_filter_samples", "hrt_scene_filter_ms", "hrt_multi_filter_ms",
               "hrt_develop_defaults", "hrt_develop_workspace_bytes", "hrt_develop_device", "hrt_develop"]
HOST_SYMBOLS = ["hrt_host_load_yaml", "hrt_host_free", "hrt_host_flat", "hrt_host_film", "hrt_host_camera", "hrt_host_bvh_depth",
                "hrt_default_params", "hrt_asset_write_teapot_obj", "hrt_asset_write_bust_obj", "hrt_asset_write_hall_hdr",
                "hrt_host_write_image", "hrt_host_read_hdr", "hrt_host_read_png", "hrt_host_read_jpeg", "hrt_host_write_hdr", "hrt_host_write_pfm", "hrt_host_read_pfm", "hrt_host_last_error", "hrt_host_set_bvh_builder"]


def _load(path):
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it first (python -c 'import __graft_entry__ as g; g.build()' or `make`). "
                          "There is no fallback implementation.")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


_host = _load(HOST_LIB_PATH)
_hip = _load(HIP_LIB_PATH)

_fp = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)
_vp = C.c_void_p

_hip.hrt_status_str.restype = C.c_char_p
_hip.hrt_last_error.restype = C.c_char_p
_hip.hrt_version.restype = C.c_char_p
_hip.hrt_device_count.argtypes = [C.POINTER(C.c_int)]
_hip.hrt_scene_create.argtypes = [C.POINTER(FlatScene), C.c_int, C.POINTER(_vp)]
_hip.hrt_scene_destroy.argtypes = [_vp]
_hip.hrt_scene_destroy.restype = None
_hip.hrt_render_tile.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), Rect, _fp, C.POINTER(Stats)]
_hip.hrt_render_stripes_device.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, _vp, _vp]
_hip.hrt_render_stripes.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, _fp, C.POINTER(Stats)]
_hip.hrt_render_stripes_accumulate_device.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, _vp,
                                                      C.c_int32, C.c_int32, _vp]
_hip.hrt_render_stripes_accumulate.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, _fp,
                                               C.c_int32, C.c_int32, C.POINTER(Stats)]
_hip.hrt_render_stripes_adaptive_device.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32,
                                                   C.POINTER(Adaptive), _vp, _vp, _vp, C.c_int32, C.POINTER(C.c_int64), _vp]
_hip.hrt_render_stripes_adaptive.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32,
                                            C.POINTER(Adaptive), _fp, _fp, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64),
                                            C.POINTER(Stats)]
_hip.hrt_adaptive_mean_device.argtypes = [_vp, _vp, _vp, C.c_int64, _vp, _vp]
_hip.hrt_stripe_rows.argtypes = [C.c_int32] * 4
_hip.hrt_stripe_rows.restype = C.c_int32
_hip.hrt_stripe_row_index.argtypes = [C.c_int32] * 5
_hip.hrt_stripe_row_index.restype = C.c_int32
_hip.hrt_scene_stats.argtypes = [_vp, C.POINTER(Stats)]
_hip.hrt_resolve_u8.argtypes = [_vp, _fp, C.c_int64, _u8p]
_hip.hrt_resolve_u8_device.argtypes = [_vp, _vp, C.c_int64, _vp, _vp]
_hip.hrt_closest_hit.argtypes = [_vp, C.POINTER(Params), C.c_int64, _fp, _fp, C.c_float, C.c_float, C.c_uint32, C.POINTER(Hit)]
_hip.hrt_multi_create.argtypes = [C.POINTER(FlatScene), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(_vp)]
_hip.hrt_multi_destroy.argtypes = [_vp]
_hip.hrt_multi_destroy.restype = None
_hip.hrt_multi_devices.argtypes = [_vp]
_hip.hrt_multi_devices.restype = C.c_int32
_hip.hrt_multi_uses_rccl.argtypes = [_vp]
_hip.hrt_multi_uses_rccl.restype = C.c_int32
_hip.hrt_multi_render.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _u8p, C.POINTER(Stats)]
_hip.hrt_scene_set_roulette.argtypes = [_vp, C.c_int32, C.c_float]
_hip.hrt_multi_set_roulette.argtypes = [_vp, C.c_int32, C.c_float]
_hip.hrt_render_aov_tile.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), Rect, _fp]
_hip.hrt_render_aov_stripes_device.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, _vp]
_hip.hrt_render_aov_stripes.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32, C.c_int32]
_hip.hrt_aov_ids_bytes.argtypes = [C.c_int64]
_hip.hrt_aov_ids_bytes.restype = C.c_uint64
_hip.hrt_render_aov_ids_tile.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), Rect, _vp]
_hip.hrt_render_aov_ids_stripes_device.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, _vp]
_hip.hrt_render_aov_ids_stripes.argtypes = [_vp, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32]
_hip.hrt_denoise_defaults.argtypes = [C.POINTER(DenoiseParams)]
_hip.hrt_denoise_defaults.restype = None
_hip.hrt_denoise_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
_hip.hrt_denoise_workspace_bytes.restype = C.c_uint64
_hip.hrt_denoise_device.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(DenoiseParams), _vp, _vp, _vp, _vp, _vp, _vp]
_hip.hrt_denoise.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(DenoiseParams), _fp, _fp, _fp, _fp]
_hip.hrt_denoise_resolve_u8.argtypes = [C.c_int, _fp, C.c_int64, _u8p]
_hip.hrt_variance_state_bytes.argtypes = [C.c_int64]
_hip.hrt_variance_state_bytes.restype = C.c_uint64
_hip.hrt_variance_fold_device.argtypes = [C.c_int, C.c_int64, _vp, C.c_float, C.c_int32, C.c_int32, _vp, _vp]
_hip.hrt_variance_finish_device.argtypes = [C.c_int, C.c_int64, _vp, C.c_int32, C.c_int32, _vp, _vp]
_hip.hrt_adaptive_variance_device.argtypes = [C.c_int, C.c_int64, _vp, _vp, _vp, _vp, _vp]
_hip.hrt_variance_fold.argtypes = [C.c_int, C.c_int64, _fp, C.c_float, C.c_int32, C.c_int32, _fp]
_hip.hrt_variance_finish.argtypes = [C.c_int, C.c_int64, _fp, C.c_int32, C.c_int32, _fp]
_hip.hrt_adaptive_variance.argtypes = [C.c_int, C.c_int64, _fp, _fp, C.POINTER(C.c_int32), _fp]
_hip.hrt_despeckle_defaults.argtypes = [C.POINTER(DespeckleParams)]
_hip.hrt_despeckle_defaults.restype = None
_hip.hrt_despeckle_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
_hip.hrt_despeckle_workspace_bytes.restype = C.c_uint64
_hip.hrt_despeckle_device.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(DespeckleParams), _vp, _vp, _vp, _vp, _vp, _vp]
_hip.hrt_despeckle.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(DespeckleParams), _fp, _fp, _fp, _fp]
_hip.hrt_scene_set_filter.argtypes = [_vp, C.c_int32, C.c_float]
_hip.hrt_multi_set_filter.argtypes = [_vp, C.c_int32, C.c_float]
_hip.hrt_scene_filter_ms.argtypes = [_vp, C.POINTER(C.c_double)]
_hip.hrt_multi_filter_ms.argtypes = [_vp, C.POINTER(C.c_double)]
_hip.hrt_filter_samples.argtypes = [C.c_int, C.c_int32, C.c_float, C.c_int32, C.c_int32, Rect, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, _fp, _fp]
_hip.hrt_develop_defaults.argtypes = [C.POINTER(DevelopParams)]
_hip.hrt_develop_defaults.restype = None
_hip.hrt_develop_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
_hip.hrt_develop_workspace_bytes.restype = C.c_uint64
_hip.hrt_develop_device.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(DevelopParams), _vp, _vp, _vp, _vp, _vp, _vp]
_hip.hrt_develop.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(DevelopParams), _fp, _fp, C.POINTER(DevelopInfo), C.POINTER(C.c_uint32)]
_hip.hrt_math_probe.argtypes = [C.c_int, C.c_int32, C.c_int64, _fp, _fp, _fp]
_hip.hrt_sampler_probe.argtypes = [C.c_int, C.c_uint64, C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
_hip.hrt_env_table_build.argtypes = [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp]
_hip.hrt_emitter_table_build.argtypes = [_vp, C.POINTER(C.c_int64), _fp, _fp, _fp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]

_host.hrt_host_last_error.restype = C.c_char_p
_host.hrt_host_load_yaml.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(_vp)]
_host.hrt_host_free.argtypes = [_vp]
_host.hrt_host_free.restype = None
_host.hrt_host_flat.argtypes = [_vp]
_host.hrt_host_flat.restype = C.POINTER(FlatScene)
_host.hrt_host_film.argtypes = [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
_host.hrt_host_camera.argtypes = [_vp, C.c_int32, C.c_int32, C.POINTER(Camera)]
_host.hrt_host_bvh_depth.argtypes = [_vp, C.c_int32]
_host.hrt_host_bvh_depth.restype = C.c_int32
_host.hrt_default_params.argtypes = [C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32]
_host.hrt_default_params.restype = None
_host.hrt_asset_write_teapot_obj.argtypes = [C.c_char_p, C.c_double]
_host.hrt_asset_write_teapot_obj.restype = C.c_int64
_host.hrt_asset_write_bust_obj.argtypes = [C.c_char_p, C.c_double]
_host.hrt_asset_write_bust_obj.restype = C.c_int64
_host.hrt_asset_write_hall_hdr.argtypes = [C.c_char_p, C.c_int32, C.c_int32]
_host.hrt_host_write_image.argtypes = [C.c_char_p, _u8p, C.c_int32, C.c_int32]
_host.hrt_host_read_hdr.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp, C.c_int64]
_host.hrt_host_read_png.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _u8p, C.c_int64]
_host.hrt_host_read_jpeg.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _u8p, C.c_int64]
_host.hrt_host_write_hdr.argtypes = [C.c_char_p, _fp, C.c_int32, C.c_int32]
_host.hrt_host_write_pfm.argtypes = [C.c_char_p, _fp, C.c_int32, C.c_int32]
_host.hrt_host_read_pfm.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp, C.c_int64]


def _check(st):
    if st != HRT_OK:
        raise HrtError(st, f"{_hip.hrt_status_str(st).decode()}: {_hip.hrt_last_error().decode()}")


def _check_host(st):
    if st != HRT_OK:
        raise HrtError(st, f"{_hip.hrt_status_str(st).decode()}: {_host.hrt_host_last_error().decode()}")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a, t=_fp):
    return a.ctypes.data_as(t)


# ---------------------------------------------------------------- host side
def default_params(width, height, samples, quirks=QUIRKS_REFERENCE, seed=0, max_depth=50, stats=False, megakernel=False, timing=False,
                   thin_lens=False, progress=False, nee=False, nee_env=False, nee_emitters=False, nee_lobes=False, stratified=False,
                   roulette=False, filter=False):
    """nee: next-event estimation with MIS for the scene's rect and sphere lights (FLAG_NEE).
    nee_env: also importance-sample the environment map (FLAG_NEE_ENV); implies nee.
    nee_emitters: sample every rect, box and mesh emitter, wrapped or not, by an alias table (FLAG_NEE_EMITTERS);
    implies nee.
    nee_lobes: rough metal and medium vertices sample lights too (FLAG_NEE_LOBES); implies nee.
    stratified: the samples of a pixel from Owen-scrambled (0,2)-sequences instead of independent Philox words (FLAG_STRATIFIED,
    DESIGN.md 4.9); combines with every flag but megakernel.
    roulette: Russian roulette path termination (FLAG_ROULETTE) with the scene's parameters (DeviceScene.set_roulette /
    MultiScene.set_roulette; 3 and 0.05 by default); combines with every flag but megakernel and stats.
    filter: the film through the scene's reconstruction filter instead of the box filter (FLAG_FILTER; DeviceScene.set_filter /
    MultiScene.set_filter, Mitchell at radius 2 by default): whole-film and tile renders on one rank; not with megakernel or adaptive passes."""
    p = Params()
    _host.hrt_default_params(C.byref(p), width, height, samples)
    p.quirks = quirks
    p.seed_lo = seed & 0xFFFFFFFF
    p.seed_hi = (seed >> 32) & 0xFFFFFFFF
    p.max_depth = max_depth
    p.flags = (FLAG_STATS if stats else 0) | (FLAG_MEGAKERNEL if megakernel else 0) | (FLAG_TIMING if timing else 0) | \
              (FLAG_THIN_LENS if thin_lens else 0) | (FLAG_PROGRESS if progress else 0) | (FLAG_NEE if nee or nee_env or nee_emitters or nee_lobes else 0) | \
              (FLAG_NEE_ENV if nee_env else 0) | (FLAG_NEE_EMITTERS if nee_emitters else 0) | (FLAG_NEE_LOBES if nee_lobes else 0) | \
              (FLAG_STRATIFIED if stratified else 0) | (FLAG_ROULETTE if roulette else 0) | (FLAG_FILTER if filter else 0)
    return p


class HostScene:
    """Scene::loadScene + flatten (scene.cpp:127-379)."""

    def __init__(self, yaml_path, asset_dir=None):
        self._h = None
        h = _vp()
        _check_host(_host.hrt_host_load_yaml(os.fsencode(yaml_path), os.fsencode(asset_dir) if asset_dir else None, C.byref(h)))
        self._h = h
        self.flat_ptr = _host.hrt_host_flat(h)
        self.flat = self.flat_ptr.contents

    def close(self):
        if self._h:
            _host.hrt_host_free(self._h)
            self._h = None

    def __del__(self):
        try:                     # at interpreter shutdown the module globals may already be gone
            self.close()
        except Exception:
            pass

    @property
    def film(self):
        w, h, s = C.c_int32(), C.c_int32(), C.c_int32()
        buf = C.create_string_buffer(1024)
        _check_host(_host.hrt_host_film(self._h, C.byref(w), C.byref(h), C.byref(s), buf, 1024))
        return w.value, h.value, s.value, buf.value.decode()

    def camera(self, width=None, height=None):
        fw, fh, _, _ = self.film
        cam = Camera()
        _check_host(_host.hrt_host_camera(self._h, width or fw, height or fh, C.byref(cam)))
        return cam

    def bvh_depth(self, mesh=0):
        return _host.hrt_host_bvh_depth(self._h, mesh)

    def mesh_arrays(self, mesh=0):
        m = self.flat.meshes[mesh]
        n = m.tri_count
        pos = np.ctypeslib.as_array(self.flat.tri_pos, shape=(self.flat.n_tris * 9,))[m.tri_first * 9:(m.tri_first + n) * 9].reshape(n, 3, 3)
        nrm = np.ctypeslib.as_array(self.flat.tri_nrm, shape=(self.flat.n_tris * 9,))[m.tri_first * 9:(m.tri_first + n) * 9].reshape(n, 3, 3)
        uv = np.ctypeslib.as_array(self.flat.tri_uv, shape=(self.flat.n_tris * 6,))[m.tri_first * 6:(m.tri_first + n) * 6].reshape(n, 3, 2)
        return pos, nrm, uv


def write_teapot_obj(path, detail=1.0):
    n = _host.hrt_asset_write_teapot_obj(os.fsencode(path), detail)
    if n < 0:
        raise HrtError(HRT_ERR_IO, f"cannot write {path}")
    return n


def write_bust_obj(path, detail=1.0):
    n = _host.hrt_asset_write_bust_obj(os.fsencode(path), detail)
    if n < 0:
        raise HrtError(HRT_ERR_IO, f"cannot write {path}")
    return n


def write_hall_hdr(path, width=4096, height=2048):
    _check_host(_host.hrt_asset_write_hall_hdr(os.fsencode(path), width, height))


def write_image(path, rgb8):
    a = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w, _ = a.shape
    _check_host(_host.hrt_host_write_image(os.fsencode(path), _ptr(a, _u8p), w, h))


def read_hdr(path):
    w, h = C.c_int32(), C.c_int32()
    _check_host(_host.hrt_host_read_hdr(os.fsencode(path), C.byref(w), C.byref(h), None, 0))
    out = np.empty((h.value, w.value, 3), dtype=np.float32)
    _check_host(_host.hrt_host_read_hdr(os.fsencode(path), C.byref(w), C.byref(h), _ptr(out), out.size))
    return out


def write_hdr(path, rgb):
    a = _f32(rgb)
    h, w, _ = a.shape
    _check_host(_host.hrt_host_write_hdr(os.fsencode(path), _ptr(a), w, h))


def read_jpeg(path):
    w, h = C.c_int32(), C.c_int32()
    _check_host(_host.hrt_host_read_jpeg(os.fsencode(path), C.byref(w), C.byref(h), None, 0))
    out = np.empty((h.value, w.value, 3), dtype=np.uint8)
    _check_host(_host.hrt_host_read_jpeg(os.fsencode(path), C.byref(w), C.byref(h), _ptr(out, _u8p), out.size))
    return out


def write_pfm(path, rgb):
    a = _f32(rgb)
    h, w, _ = a.shape
    _check_host(_host.hrt_host_write_pfm(os.fsencode(path), _ptr(a), w, h))


def read_pfm(path):
    w, h = C.c_int32(), C.c_int32()
    _check_host(_host.hrt_host_read_pfm(os.fsencode(path), C.byref(w), C.byref(h), None, 0))
    out = np.empty((h.value, w.value, 3), dtype=np.float32)
    _check_host(_host.hrt_host_read_pfm(os.fsencode(path), C.byref(w), C.byref(h), _ptr(out), out.size))
    return out


def read_png(path):
    w, h = C.c_int32(), C.c_int32()
    _check_host(_host.hrt_host_read_png(os.fsencode(path), C.byref(w), C.byref(h), None, 0))
    out = np.empty((h.value, w.value, 3), dtype=np.uint8)
    _check_host(_host.hrt_host_read_png(os.fsencode(path), C.byref(w), C.byref(h), _ptr(out, _u8p), out.size))
    return out


# ---------------------------------------------------------------- device side
def device_count():
    n = C.c_int()
    st = _hip.hrt_device_count(C.byref(n))
    return n.value if st == HRT_OK else 0


def use_device_bvh_builder(enable=True, device=0, algo="lbvh"):
    """hrt_host_set_bvh_builder: scenes loaded from now on get their meshes' culling trees from the GPU -- hrt_bvh_build_device
    (algo "lbvh": a Morton-ordered LBVH, fastest) or hrt_bvh_build_sah ("sah": the host builder's own binned-SAH tree, built on
    the device) -- instead of the host's builder."""
    _host.hrt_host_set_bvh_builder.argtypes = [C.c_void_p, C.c_int]
    _host.hrt_host_set_bvh_builder.restype = None
    fn = {"lbvh": _hip.hrt_bvh_build_device, "sah": _hip.hrt_bvh_build_sah}[algo]
    _host.hrt_host_set_bvh_builder(C.cast(fn, C.c_void_p) if enable else None, device)


def bvh_build_device(tri_pos, max_leaf=2, device=0, algo="lbvh"):
    """hrt_bvh_build_device on an (n, 9) float32 array: (nodes as an (n_nodes, 16) uint32 view of hrt_bvh_node, order, depth)."""
    pos = np.ascontiguousarray(tri_pos, dtype=np.float32).reshape(-1, 9)
    n = pos.shape[0]
    nodes = np.zeros((max(n - 1, 1), 16), dtype=np.uint32)
    order = np.zeros(n, dtype=np.uint32)
    n_nodes, depth = C.c_uint32(), C.c_int32()
    f = {"lbvh": _hip.hrt_bvh_build_device, "sah": _hip.hrt_bvh_build_sah}[algo]
    f.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    _check(f(device, pos.ctypes.data, n, max_leaf, nodes.ctypes.data, C.addressof(n_nodes), order.ctypes.data, C.addressof(depth)))
    return nodes[:n_nodes.value], order, depth.value


def env_table_build(texels):
    """FLAG_NEE_ENV's sampling table of an environment map (hrt_env_table_build), built on the current device by the
    kernels hrt_scene_create runs.  texels: [H, W, C >= 3] fp32, rows from the top.  Returns (marginal [H + 1], conditional [H, W + 1])
    fp32 CDFs, or None when the map has no table (total weight 0 or not finite)."""
    t = np.ascontiguousarray(texels, np.float32)
    if t.ndim != 3 or t.shape[2] < 3:
        raise ValueError("texels must be [H, W, C >= 3]")
    H, W, ch = t.shape
    marg = np.zeros(H + 1, np.float32)
    cond = np.zeros((H, W + 1), np.float32)
    _check(_hip.hrt_env_table_build(_ptr(t), W, H, ch, _ptr(marg), _ptr(cond)))
    return None if marg[H] == 0.0 else (marg, cond)


def emitter_table_build(flat_ptr):
    """FLAG_NEE_EMITTERS' emitter table of a flattened scene (hrt_emitter_table_build), host only.  Returns a dict of
    numpy arrays: rec [n, 16] fp32 (the 4 float4 of hrt_emitters.h), shade [n, 4] fp32, thresh [n] fp32, alias [n] int32, base
    [n_prims] int32, plus the record fields prim, kind, sub (int32) and p_sel (fp32); n = 0 when the scene has no table."""
    n = C.c_int64(0)
    _check(_hip.hrt_emitter_table_build(flat_ptr, C.byref(n), None, None, None, None, None))
    n_prims = C.cast(flat_ptr, C.POINTER(FlatScene)).contents.n_prims
    k = max(1, n.value)
    rec = np.zeros((k, 16), np.float32)
    shade = np.zeros((k, 4), np.float32)
    thresh = np.zeros(k, np.float32)
    alias = np.zeros(k, np.int32)
    base = np.zeros(max(1, n_prims), np.int32)
    _check(_hip.hrt_emitter_table_build(flat_ptr, C.byref(n), _ptr(rec), _ptr(shade), _ptr(thresh), _ptr(alias, C.POINTER(C.c_int32)),
                                        _ptr(base, C.POINTER(C.c_int32))))
    m = n.value
    rec, shade, thresh, alias, base = rec[:m], shade[:m], thresh[:m], alias[:m], base[:n_prims]
    bits = rec.view(np.int32)
    return {"rec": rec, "shade": shade, "thresh": thresh, "alias": alias, "base": base,
            "prim": bits[:, 0].copy(), "kind": bits[:, 1].copy(), "p_sel": rec[:, 2].copy(), "sub": bits[:, 3].copy()}


def stripe_rows(height, rows_per_block, rank, n_ranks):
    return _hip.hrt_stripe_rows(height, rows_per_block, rank, n_ranks)


def stripe_row_index(height, rows_per_block, rank, n_ranks, local_row):
    return _hip.hrt_stripe_row_index(height, rows_per_block, rank, n_ranks, local_row)


def stripe_row_indices(height, rows_per_block, rank, n_ranks):
    n = stripe_rows(height, rows_per_block, rank, n_ranks)
    return np.array([_hip.hrt_stripe_row_index(height, rows_per_block, rank, n_ranks, i) for i in range(n)], dtype=np.int64)


def split_aov(buf):
    """A raw feature buffer [..., 8] (hrt_render_aov_*: albedo r g b, alpha, normal x y z, depth per pixel) as a dict of views:
    albedo [..., 3], alpha [...], normal [..., 3], depth [...]."""
    if buf.shape[-1] != 8:
        raise ValueError("a feature buffer has 8 floats per pixel")
    return {"albedo": buf[..., 0:3], "alpha": buf[..., 3], "normal": buf[..., 4:7], "depth": buf[..., 7]}


# One pixel of the buffer of hrt_render_aov_ids_* (include/hrt.h): 80 bytes, five groups of 16.
AOV_IDS_DTYPE = np.dtype([("position", "<f4", 4), ("object_id", "<i4", 4), ("object_coverage", "<f4", 4), ("material_id", "<i4", 4),
                          ("material_coverage", "<f4", 4)])
assert AOV_IDS_DTYPE.itemsize == 80
AOV_ID_SLOTS, AOV_ID_RANKS = 8, 4
AOV_ID_UNUSED = -2 ** 31       # the id of a rank beyond the used slots (INT32_MIN); its coverage is +0


def aov_ids_bytes(n_pixels):
    return int(_hip.hrt_aov_ids_bytes(n_pixels))


def split_aov_ids(buf):
    """A raw id buffer [...] of AOV_IDS_DTYPE (hrt_render_aov_ids_*) as a dict of views: position [..., 3] fp32, object_id [..., 4]
    int32, object_coverage [..., 4] fp32, material_id [..., 4] int32, material_coverage [..., 4] fp32; rank 0 first."""
    if buf.dtype != AOV_IDS_DTYPE:
        raise ValueError("an id buffer has dtype AOV_IDS_DTYPE (80 bytes per pixel)")
    return {"position": buf["position"][..., 0:3], "object_id": buf["object_id"], "object_coverage": buf["object_coverage"],
            "material_id": buf["material_id"], "material_coverage": buf["material_coverage"]}


def matte(ids, coverage, wanted):
    """The matte of the ids in `wanted` (an int or an iterable of ints): ids [..., 4] int32 and coverage [..., 4] fp32 of one id kind
    (split_aov_ids) -> [...] fp32, the sum of the coverages of the ranks whose id is wanted, added in rank order in fp32 from +0."""
    ids, coverage = np.asarray(ids), np.asarray(coverage, dtype=np.float32)
    if ids.shape != coverage.shape or ids.shape[-1] != AOV_ID_RANKS:
        raise ValueError("matte takes ids and coverage of the same shape [..., 4]")
    wanted = np.atleast_1d(np.asarray(wanted, dtype=np.int64)).ravel()
    out = np.zeros(ids.shape[:-1], dtype=np.float32)
    for k in range(AOV_ID_RANKS):
        out = out + np.where(np.isin(ids[..., k], wanted), coverage[..., k], np.float32(0.0)).astype(np.float32)
    return out


def denoise_defaults(**params):
    """hrt_denoise_defaults, then the given fields (iterations, normal_squarings, sigma_l, sigma_z, albedo_floor) -> DenoiseParams."""
    p = DenoiseParams()
    _hip.hrt_denoise_defaults(C.byref(p))
    names = [n for n, _ in DenoiseParams._fields_]
    for k, v in params.items():
        if k not in names:
            raise TypeError(f"hrt_denoise_params has no field {k!r}")
        setattr(p, k, v)
    return p


def denoise_workspace_bytes(width, height):
    return int(_hip.hrt_denoise_workspace_bytes(width, height))


def denoise(rgb, aov, variance=None, device=0, **params):
    """The guided denoiser (hrt_denoise, include/hrt.h) on `device`: the linear film rgb [H, W, 3], the raw feature
    buffer aov [H, W, 8] of render_aov_* (the dict of split_aov is accepted too) and, optionally, the variance of every pixel's mean
    luminance [H, W] -> the filtered film [H, W, 3].  **params: fields of DenoiseParams that differ from the defaults."""
    if isinstance(aov, dict):
        aov = np.concatenate([aov["albedo"], aov["alpha"][..., None], aov["normal"], aov["depth"][..., None]], axis=-1)
    rgb, aov = _f32(rgb), _f32(aov)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or aov.shape != rgb.shape[:2] + (8,):
        raise ValueError("denoise takes rgb [H, W, 3] and aov [H, W, 8]")
    H, W = rgb.shape[:2]
    var = None
    if variance is not None:
        var = _f32(variance)
        if var.shape != (H, W):
            raise ValueError("variance must be [H, W]")
    p = denoise_defaults(**params)
    out = np.empty_like(rgb)
    _check(_hip.hrt_denoise(device, W, H, C.byref(p), _ptr(rgb), _ptr(aov), _ptr(var) if var is not None else None, _ptr(out)))
    return out


def denoise_device(width, height, d_rgb_ptr, d_aov_ptr, d_out_ptr, d_workspace_ptr, d_var_ptr=None, device=0, stream=0, params=None):
    """Asynchronous (hrt_denoise_device): raw device pointers (e.g. torch tensors' .data_ptr()) to rgb [H, W, 3], aov [H, W, 8], out
    [H, W, 3] (may be rgb itself), a workspace of denoise_workspace_bytes(width, height) and, optionally, the variance [H, W]."""
    p = params if params is not None else denoise_defaults()
    _check(_hip.hrt_denoise_device(device, width, height, C.byref(p), _vp(d_rgb_ptr), _vp(d_aov_ptr), _vp(d_var_ptr) if d_var_ptr else None,
                                   _vp(d_out_ptr), _vp(d_workspace_ptr), _vp(stream)))


def denoise_resolve_u8(rgb_linear, device=0):
    """hrt_denoise_resolve_u8: DeviceScene.resolve_u8 without a scene -> uint8 array of the same shape."""
    a = _f32(rgb_linear)
    out = np.empty(a.shape, dtype=np.uint8)
    _check(_hip.hrt_denoise_resolve_u8(device, _ptr(a), a.size // 3, _ptr(out, _u8p)))
    return out


def _filter_kind(kind):
    if isinstance(kind, str):
        if kind not in FILTER_KINDS:
            raise ValueError(f"filter kind must be one of {sorted(FILTER_KINDS)}")
        return FILTER_KINDS[kind]
    return int(kind)


def filter_samples(rad, kind="mitchell", radius=0.0, width=None, height=None, rect=None, seed=0, stratified=False, device=0):
    """The reconstruction filter on stored samples (hrt_filter_samples, include/hrt.h), on `device`: rad [S, h, w, 3], the
    value of each of the S samples of every pixel of `rect` = (x0, y0, w, h) of the width x height film (default: the whole film, w x h)
    -> the finished film [h, w, 3].  kind: "tent", "bspline", "mitchell" or a FILTER_* value; radius <= 0: the kind's default.  The
    jitters are those of a render with `seed` and, with stratified, FLAG_STRATIFIED."""
    rad = _f32(rad)
    if rad.ndim != 4 or rad.shape[3] != 3:
        raise ValueError("filter_samples takes rad [samples, h, w, 3]")
    S, h, w = rad.shape[:3]
    if rect is None:
        rect = (0, 0, w, h)
    if tuple(rect[2:]) != (w, h):
        raise ValueError("rad must hold rect's h x w pixels")
    W = w if width is None else width
    H = h if height is None else height
    out = np.empty((h, w, 3), np.float32)
    _check(_hip.hrt_filter_samples(device, _filter_kind(kind), radius, W, H, Rect(*rect), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                                   1 if stratified else 0, S, _ptr(rad), _ptr(out)))
    return out


def despeckle_defaults(**params):
    """hrt_despeckle_defaults, then the given fields (radius, rank, ratio, gate_z, repair_invalid) -> DespeckleParams."""
    p = DespeckleParams()
    _hip.hrt_despeckle_defaults(C.byref(p))
    names = [n for n, _ in DespeckleParams._fields_]
    for k, v in params.items():
        if k not in names:
            raise TypeError(f"hrt_despeckle_params has no field {k!r}")
        setattr(p, k, v)
    return p


def despeckle_workspace_bytes(width, height):
    return int(_hip.hrt_despeckle_workspace_bytes(width, height))


def despeckle(rgb, variance=None, device=0, return_map=False, **params):
    """The outlier filter (hrt_despeckle, include/hrt.h) on `device`: the linear film rgb [H, W, 3] and, optionally, the
    variance of every pixel's mean luminance [H, W] (without it the variance gate is off) -> the filtered film [H, W, 3]; with
    return_map also the map [H, W]: 1 - s for an outlier, -1 for a repaired pixel, 0 elsewhere.  **params: fields of DespeckleParams
    that differ from the defaults."""
    rgb = _f32(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("despeckle takes rgb [H, W, 3]")
    H, W = rgb.shape[:2]
    var = None
    if variance is not None:
        var = _f32(variance)
        if var.shape != (H, W):
            raise ValueError("variance must be [H, W]")
    p = despeckle_defaults(**params)
    out = np.empty_like(rgb)
    dmap = np.empty((H, W), np.float32) if return_map else None
    _check(_hip.hrt_despeckle(device, W, H, C.byref(p), _ptr(rgb), _ptr(var) if var is not None else None, _ptr(out),
                              _ptr(dmap) if dmap is not None else None))
    return (out, dmap) if return_map else out


def despeckle_device(width, height, d_rgb_ptr, d_out_ptr, d_workspace_ptr, d_var_ptr=None, d_map_ptr=None, device=0, stream=0, params=None):
    """Asynchronous (hrt_despeckle_device): raw device pointers (e.g. torch tensors' .data_ptr()) to rgb [H, W, 3], out [H, W, 3] (not
    rgb itself), a workspace of despeckle_workspace_bytes(width, height) and, optionally, the variance [H, W] and the map [H, W]."""
    p = params if params is not None else despeckle_defaults()
    _check(_hip.hrt_despeckle_device(device, width, height, C.byref(p), _vp(d_rgb_ptr), _vp(d_var_ptr) if d_var_ptr else None, _vp(d_out_ptr),
                                     _vp(d_map_ptr) if d_map_ptr else None, _vp(d_workspace_ptr), _vp(stream)))


def develop_defaults(**params):
    """hrt_develop_defaults, then the given fields (bloom_levels, bloom_strength, exposure_mode, exposure_ev, key, meter_low, meter_high,
    meter_floor, ev_min, ev_max) -> DevelopParams.  The defaults are the identity."""
    p = DevelopParams()
    _hip.hrt_develop_defaults(C.byref(p))
    names = [n for n, _ in DevelopParams._fields_]
    for k, v in params.items():
        if k not in names:
            raise TypeError(f"hrt_develop_params has no field {k!r}")
        setattr(p, k, v)
    return p


def develop_workspace_bytes(width, height, levels):
    return int(_hip.hrt_develop_workspace_bytes(width, height, levels))


def develop(rgb, device=0, return_info=False, return_histogram=False, **params):
    """The develop stage (hrt_develop, include/hrt.h) on `device`: the linear film rgb [H, W, 3] -> the developed film
    [H, W, 3], after a pyramid bloom (bloom_levels, bloom_strength) and an exposure (exposure_mode = EXPOSURE_NONE, EXPOSURE_MANUAL with
    exposure_ev, or EXPOSURE_AUTO, metered from the film).  With return_info also a DevelopInfo (mean_ev, scale, metered, levels), with
    return_histogram also the 2048 bin counts of the meter as uint32.  **params: fields of DevelopParams that differ from the defaults."""
    rgb = _f32(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("develop takes rgb [H, W, 3]")
    H, W = rgb.shape[:2]
    p = develop_defaults(**params)
    out = np.empty_like(rgb)
    info = DevelopInfo() if return_info else None
    hist = np.zeros(DEVELOP_BINS, np.uint32) if return_histogram else None
    _check(_hip.hrt_develop(device, W, H, C.byref(p), _ptr(rgb), _ptr(out), C.byref(info) if info is not None else None,
                            hist.ctypes.data_as(C.POINTER(C.c_uint32)) if hist is not None else None))
    res = (out,) + ((info,) if return_info else ()) + ((hist,) if return_histogram else ())
    return res if len(res) > 1 else out


def develop_device(width, height, d_rgb_ptr, d_out_ptr, d_workspace_ptr, d_info_ptr=None, d_hist_ptr=None, device=0, stream=0, params=None):
    """Asynchronous (hrt_develop_device): raw device pointers (e.g. torch tensors' .data_ptr()) to rgb [H, W, 3], out [H, W, 3] (which may
    be rgb itself), a workspace of develop_workspace_bytes(width, height, params.bloom_levels) and, optionally, room for one DevelopInfo
    (24 bytes, 8-byte aligned) and for the 2048 uint32 bin counts."""
    p = params if params is not None else develop_defaults()
    _check(_hip.hrt_develop_device(device, width, height, C.byref(p), _vp(d_rgb_ptr), _vp(d_out_ptr), _vp(d_info_ptr) if d_info_ptr else None,
                                   _vp(d_hist_ptr) if d_hist_ptr else None, _vp(d_workspace_ptr), _vp(stream)))


def variance_state_bytes(n_pixels):
    """hrt_variance_state_bytes: the bytes of the batch-means state of n_pixels pixels (8 each)."""
    return int(_hip.hrt_variance_state_bytes(n_pixels))


def variance_batches(samples, batches):
    """The sample ranges [(first, count), ...] of a render split into `batches` passes for the measured variance: range j starts at
    j * ceil(samples / batches) and the last one takes what is left (fewer than `batches` ranges when they run out first)."""
    if samples < 1 or batches < 1:
        raise ValueError("samples and batches must be >= 1")
    step = -(-samples // batches)
    return [(s, min(step, samples - s)) for s in range(0, samples, step)]


def variance_fold(rgb, samples_before, samples_batch, state=None, scale=1.0, device=0):
    """One fold of the measured variance (hrt_variance_fold, include/hrt.h) on `device`: rgb [..., 3] is the accumulation
    buffer after a batch of samples_batch samples that follows samples_before earlier ones; scale is 1 while it holds undivided sums and
    the sample count for the buffer whose last pass has divided.  state [..., 2] = (yprev, M2) is the array the fold before returned
    (not read, and allocated when None, for samples_before == 0).  Returns the new state, a new array."""
    rgb = _f32(rgb)
    if rgb.ndim < 1 or rgb.shape[-1] != 3:
        raise ValueError("variance_fold takes rgb [..., 3]")
    shape = rgb.shape[:-1] + (2,)
    if state is None:
        if samples_before > 0:
            raise ValueError("samples_before > 0 continues a measurement: pass the state of the folds before")
        out = np.zeros(shape, np.float32)
    else:
        out = np.array(state, dtype=np.float32, order="C")
        if out.shape != shape:
            raise ValueError("state must be [..., 2] over the pixels of rgb")
    _check(_hip.hrt_variance_fold(device, rgb.size // 3, _ptr(rgb), scale, samples_before, samples_batch, _ptr(out)))
    return out


def variance_finish(state, samples, batches, device=0):
    """hrt_variance_finish: the state [..., 2] after `batches` folds over `samples` samples -> the variance of every pixel's mean
    luminance [...], what denoise() takes as `variance`."""
    state = _f32(state)
    if state.ndim < 1 or state.shape[-1] != 2:
        raise ValueError("variance_finish takes state [..., 2]")
    var = np.empty(state.shape[:-1], np.float32)
    _check(_hip.hrt_variance_finish(device, state.size // 2, _ptr(state), samples, batches, _ptr(var)))
    return var


def adaptive_variance(sums, sq, count, device=0):
    """hrt_adaptive_variance: the variance of every pixel's mean luminance [...] from the buffers of an adaptive render, sums [..., 3],
    sq [...] and count [...] (int32); 0 where a pixel has fewer than 2 samples."""
    sums, sq = _f32(sums), _f32(sq)
    count = np.ascontiguousarray(count, dtype=np.int32)
    if sums.shape != sq.shape + (3,) or count.shape != sq.shape:
        raise ValueError("adaptive_variance takes sums [..., 3], sq [...] and count [...]")
    var = np.empty(sq.shape, np.float32)
    _check(_hip.hrt_adaptive_variance(device, sq.size, _ptr(sums), _ptr(sq), _ptr(count, C.POINTER(C.c_int32)), _ptr(var)))
    return var


def variance_fold_device(n_pixels, d_rgb_ptr, samples_before, samples_batch, d_state_ptr, scale=1.0, device=0, stream=0):
    """Asynchronous (hrt_variance_fold_device): raw device pointers (e.g. torch tensors' .data_ptr()) to rgb [n_pixels, 3] and the state
    [n_pixels, 2] (variance_state_bytes(n_pixels) bytes, 8-byte aligned)."""
    _check(_hip.hrt_variance_fold_device(device, n_pixels, _vp(d_rgb_ptr), scale, samples_before, samples_batch, _vp(d_state_ptr), _vp(stream)))


def variance_finish_device(n_pixels, d_state_ptr, samples, batches, d_var_ptr, device=0, stream=0):
    """Asynchronous (hrt_variance_finish_device): the state [n_pixels, 2] -> the variance [n_pixels]."""
    _check(_hip.hrt_variance_finish_device(device, n_pixels, _vp(d_state_ptr), samples, batches, _vp(d_var_ptr), _vp(stream)))


def adaptive_variance_device(n_pixels, d_sums_ptr, d_sq_ptr, d_count_ptr, d_var_ptr, device=0, stream=0):
    """Asynchronous (hrt_adaptive_variance_device): the adaptive render's device buffers -> the variance [n_pixels]."""
    _check(_hip.hrt_adaptive_variance_device(device, n_pixels, _vp(d_sums_ptr), _vp(d_sq_ptr), _vp(d_count_ptr), _vp(d_var_ptr), _vp(stream)))


class DeviceScene:
    """hrt_scene: the flat scene resident on one GPU."""

    def __init__(self, flat, device=0):
        self._h = None
        h = _vp()
        flat_ptr = flat if isinstance(flat, C.POINTER(FlatScene)) else C.pointer(flat)
        _check(_hip.hrt_scene_create(flat_ptr, device, C.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if self._h:
            _hip.hrt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_roulette(self, first_bounce=ROULETTE_FIRST_BOUNCE, q_floor=ROULETTE_Q_FLOOR):
        """FLAG_ROULETTE's parameters for the renders of this scene that follow (hrt_scene_set_roulette): roulette from a path's
        first_bounce-th scatter on, no survival probability below q_floor.  HrtError (HRT_ERR_INVALID) for first_bounce < 0 or a q_floor
        outside (0, 1]."""
        _check(_hip.hrt_scene_set_roulette(self._h, first_bounce, q_floor))

    def set_filter(self, kind="mitchell", radius=0.0):
        """FLAG_FILTER's parameters for the renders of this scene that follow (hrt_scene_set_filter): kind "tent", "bspline", "mitchell"
        or a FILTER_* value; radius in pixels, <= 0: the kind's default (1, 2, 2).  HrtError (HRT_ERR_INVALID) for an unknown kind, a
        NaN radius or one outside [0.5, 2.5]."""
        _check(_hip.hrt_scene_set_filter(self._h, _filter_kind(kind), radius))

    def filter_ms(self):
        """The time the filter's own kernels took in this scene's render calls since the last call of this, in ms (hrt_scene_filter_ms)."""
        ms = C.c_double(0.0)
        _check(_hip.hrt_scene_filter_ms(self._h, C.byref(ms)))
        return ms.value

    def render_tile(self, cam, params, rect=None):
        """-> (h, w, 3) fp32 linear film tile, Stats."""
        if rect is None:
            rect = Rect(0, 0, params.width, params.height)
        elif not isinstance(rect, Rect):
            rect = Rect(*rect)
        out = np.empty((rect.h, rect.w, 3), dtype=np.float32)
        st = Stats()
        _check(_hip.hrt_render_tile(self._h, C.byref(cam), C.byref(params), rect, _ptr(out), C.byref(st)))
        return out, st

    def progress(self):
        """(paths ended, paths of the call) of the render call with FLAG_PROGRESS that is running, or ran last, on this scene
        (hrt_scene_progress: a plain read of host-mapped memory, callable from another thread while the render runs)."""
        d, t = C.c_uint64(0), C.c_uint64(0)
        _hip.hrt_scene_progress.argtypes = [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _check(_hip.hrt_scene_progress(self._h, C.byref(d), C.byref(t)))
        return d.value, t.value

    def render_stripes(self, cam, params, rows_per_block, rank, n_ranks):
        rows = stripe_rows(params.height, rows_per_block, rank, n_ranks)
        out = np.empty((rows, params.width, 3), dtype=np.float32)
        st = Stats()
        _check(_hip.hrt_render_stripes(self._h, C.byref(cam), C.byref(params), rows_per_block, rank, n_ranks, _ptr(out), C.byref(st)))
        return out, st

    def render_stripes_device(self, cam, params, rows_per_block, rank, n_ranks, d_out_ptr, stream=0):
        """Asynchronous: d_out_ptr is a device pointer (e.g. torch tensor .data_ptr()), stream a hipStream_t value."""
        _check(_hip.hrt_render_stripes_device(self._h, C.byref(cam), C.byref(params), rows_per_block, rank, n_ranks,
                                              _vp(d_out_ptr), _vp(stream)))

    def render_stripes_accumulate(self, cam, params, rows_per_block, rank, n_ranks, accum, sample_first, sample_count):
        """Progressive pass: adds samples [sample_first, sample_first + sample_count) to the host array `accum`
        (rows x W x 3 float32, running sums; divided by params.samples by the pass that reaches it)."""
        assert accum.dtype == np.float32 and accum.flags["C_CONTIGUOUS"]
        st = Stats()
        _check(_hip.hrt_render_stripes_accumulate(self._h, C.byref(cam), C.byref(params), rows_per_block, rank, n_ranks, _ptr(accum),
                                                  sample_first, sample_count, C.byref(st)))
        return st

    def render_stripes_accumulate_device(self, cam, params, rows_per_block, rank, n_ranks, d_accum_ptr, sample_first, sample_count, stream=0):
        _check(_hip.hrt_render_stripes_accumulate_device(self._h, C.byref(cam), C.byref(params), rows_per_block, rank, n_ranks,
                                                         _vp(d_accum_ptr), sample_first, sample_count, _vp(stream)))

    def render_stripes_with_variance(self, cam, params, batches=4, rows_per_block=8, rank=0, n_ranks=1):
        """The film stripes of render_stripes and the measured variance of every pixel's mean luminance, device
        resident: hrt_render_stripes_accumulate_device over the sample ranges of variance_batches(params.samples, batches) with an
        hrt_variance_fold_device after each and an hrt_variance_finish_device at the end, all on one stream of a torch device buffer
        with no host round trip in between.  -> (film [rows, W, 3], var [rows, W]) fp32; the film is render_stripes' bits.
        ValueError when fewer than two batches exist (params.samples < 2 or batches < 2)."""
        import torch
        ranges = variance_batches(params.samples, batches)
        if len(ranges) < 2:
            raise ValueError("the measured variance needs at least two batches: samples >= 2 and batches >= 2")
        rows = stripe_rows(params.height, rows_per_block, rank, n_ranks)
        n = rows * params.width
        dev = torch.device("cuda", self.device)
        accum = torch.empty((rows, params.width, 3), dtype=torch.float32, device=dev)
        state = torch.empty((rows, params.width, 2), dtype=torch.float32, device=dev)
        var = torch.empty((rows, params.width), dtype=torch.float32, device=dev)
        if n == 0:
            return accum.cpu().numpy(), var.cpu().numpy()
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            s = stream.cuda_stream
            for first, count in ranges:
                self.render_stripes_accumulate_device(cam, params, rows_per_block, rank, n_ranks, accum.data_ptr(), first, count, stream=s)
                last = first + count == params.samples
                variance_fold_device(n, accum.data_ptr(), first, count, state.data_ptr(), scale=float(params.samples) if last else 1.0,
                                     device=self.device, stream=s)
            variance_finish_device(n, state.data_ptr(), params.samples, len(ranges), var.data_ptr(), device=self.device, stream=s)
        stream.synchronize()
        return accum.cpu().numpy(), var.cpu().numpy()

    def render_stripes_adaptive(self, cam, params, rows_per_block, rank, n_ranks, adaptive, pass_index, sums=None, sq=None, count=None):
        """One adaptive pass (hrt_render_stripes_adaptive) -> (sums, sq, count, active, Stats).  Pass 0 allocates the buffers when
        they are not given (rows x W x 3 float32, rows x W float32, rows x W int32, stripe layout); later passes continue the ones
        returned.  active = pixels rendered in this pass (0: the render is finished)."""
        rows = stripe_rows(params.height, rows_per_block, rank, n_ranks)
        if sums is None:
            sums = np.empty((rows, params.width, 3), dtype=np.float32)
        if sq is None:
            sq = np.empty((rows, params.width), dtype=np.float32)
        if count is None:
            count = np.zeros((rows, params.width), dtype=np.int32)
        for a, dt, n in ((sums, np.float32, rows * params.width * 3), (sq, np.float32, rows * params.width), (count, np.int32, rows * params.width)):
            assert a.dtype == dt and a.flags["C_CONTIGUOUS"] and a.size == n
        if not isinstance(adaptive, Adaptive):
            adaptive = Adaptive(*adaptive)
        active = C.c_int64(0)
        st = Stats()
        _check(_hip.hrt_render_stripes_adaptive(self._h, C.byref(cam), C.byref(params), rows_per_block, rank, n_ranks, C.byref(adaptive),
                                                _ptr(sums), _ptr(sq), _ptr(count, C.POINTER(C.c_int32)), pass_index, C.byref(active),
                                                C.byref(st)))
        return sums, sq, count, active.value, st

    def render_stripes_adaptive_device(self, cam, params, rows_per_block, rank, n_ranks, adaptive, d_sums_ptr, d_sq_ptr, d_count_ptr,
                                       pass_index, stream=0):
        """Device-buffer pass (hrt_render_stripes_adaptive_device) -> active pixels of the pass."""
        if not isinstance(adaptive, Adaptive):
            adaptive = Adaptive(*adaptive)
        active = C.c_int64(0)
        _check(_hip.hrt_render_stripes_adaptive_device(self._h, C.byref(cam), C.byref(params), rows_per_block, rank, n_ranks,
                                                       C.byref(adaptive), _vp(d_sums_ptr), _vp(d_sq_ptr), _vp(d_count_ptr), pass_index,
                                                       C.byref(active), _vp(stream)))
        return active.value

    def adaptive_mean_device(self, d_sums_ptr, d_count_ptr, n_pixels, d_mean_ptr, stream=0):
        _check(_hip.hrt_adaptive_mean_device(self._h, _vp(d_sums_ptr), _vp(d_count_ptr), n_pixels, _vp(d_mean_ptr), _vp(stream)))

    def render_adaptive(self, cam, params, adaptive, rows_per_block=8, rank=0, n_ranks=1, on_pass=None):
        """Runs adaptive passes until none is active -> (mean, count, Stats summed over the passes).  mean = sums / count
        (rows x W x 3 float32, stripe layout; the film itself for n_ranks == 1).  on_pass(pass_index, sums, count, active)
        is called after every pass that rendered."""
        sums = sq = count = None
        total = Stats()
        p = 0
        while True:
            sums, sq, count, active, st = self.render_stripes_adaptive(cam, params, rows_per_block, rank, n_ranks, adaptive, p, sums, sq, count)
            for name, _ in Stats._fields_:
                setattr(total, name, getattr(total, name) + getattr(st, name))
            if active == 0:
                break
            if on_pass is not None:
                on_pass(p, sums, count, active)
            p += 1
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = sums / count.astype(np.float32)[..., None]
        return mean, count, total

    def render_aov_tile(self, cam, params, rect=None):
        """The feature buffers of a film tile (hrt_render_aov_tile), means over samples [0, params.samples) -> a dict of
        fp32 arrays: albedo [h, w, 3], alpha [h, w], normal [h, w, 3], depth [h, w] (split_aov)."""
        if rect is None:
            rect = Rect(0, 0, params.width, params.height)
        elif not isinstance(rect, Rect):
            rect = Rect(*rect)
        out = np.empty((max(rect.h, 0), max(rect.w, 0), 8), dtype=np.float32)
        _check(_hip.hrt_render_aov_tile(self._h, C.byref(cam), C.byref(params), rect, _ptr(out)))
        return split_aov(out)

    def render_aov_stripes(self, cam, params, rows_per_block, rank, n_ranks, buf=None, sample_first=0, sample_count=-1):
        """Adds samples [sample_first, sample_first + sample_count) (-1: all that are left) to the raw feature buffer `buf`
        ([rows, W, 8] fp32, stripe layout; allocated when not given, which only a call with sample_first == 0 may ask for) and returns it (hrt_render_aov_stripes): running sums, divided by
        params.samples by the call that reaches it."""
        rows = stripe_rows(params.height, rows_per_block, rank, n_ranks)
        if buf is None:
            if sample_first > 0:
                raise ValueError("sample_first > 0 continues an accumulation: pass the buffer of the calls before")
            buf = np.empty((rows, params.width, 8), dtype=np.float32)
        assert buf.dtype == np.float32 and buf.flags["C_CONTIGUOUS"] and buf.size == rows * params.width * 8
        _check(_hip.hrt_render_aov_stripes(self._h, C.byref(cam), C.byref(params), rows_per_block, rank, n_ranks, _ptr(buf), sample_first,
                                           sample_count))
        return buf

    def render_aov_stripes_device(self, cam, params, rows_per_block, rank, n_ranks, d_buf_ptr, sample_first=0, sample_count=-1, stream=0):
        """Asynchronous: d_buf_ptr is a device pointer to rows x W x 8 floats (e.g. a torch tensor's .data_ptr())."""
        _check(_hip.hrt_render_aov_stripes_device(self._h, C.byref(cam), C.byref(params), rows_per_block, rank, n_ranks, _vp(d_buf_ptr),
                                                  sample_first, sample_count, _vp(stream)))

    def render_aov_ids_tile(self, cam, params, rect=None):
        """The id mattes and the position buffer of a film tile (hrt_render_aov_ids_tile) over samples
        [0, params.samples) -> a dict: position [h, w, 3] fp32, object_id [h, w, 4] int32, object_coverage [h, w, 4] fp32, material_id,
        material_coverage (split_aov_ids)."""
        if rect is None:
            rect = Rect(0, 0, params.width, params.height)
        elif not isinstance(rect, Rect):
            rect = Rect(*rect)
        out = np.empty((max(rect.h, 0), max(rect.w, 0)), dtype=AOV_IDS_DTYPE)
        _check(_hip.hrt_render_aov_ids_tile(self._h, C.byref(cam), C.byref(params), rect, _vp(out.ctypes.data)))
        return split_aov_ids(out)

    def render_aov_ids_stripes(self, cam, params, rows_per_block, rank, n_ranks, buf=None, sample_first=0, sample_count=-1):
        """Samples [sample_first, sample_first + sample_count) (-1: up to params.samples) of the rank's row blocks into the raw id
        buffer `buf` ([rows, W] of AOV_IDS_DTYPE, allocated when not given) and returns it (hrt_render_aov_ids_stripes).  Every call
        starts from empty tables and overwrites the buffer: there is no accumulate form."""
        rows = stripe_rows(params.height, rows_per_block, rank, n_ranks)
        if buf is None:
            buf = np.empty((rows, params.width), dtype=AOV_IDS_DTYPE)
        assert buf.dtype == AOV_IDS_DTYPE and buf.flags["C_CONTIGUOUS"] and buf.size == rows * params.width
        _check(_hip.hrt_render_aov_ids_stripes(self._h, C.byref(cam), C.byref(params), rows_per_block, rank, n_ranks, _vp(buf.ctypes.data),
                                               sample_first, sample_count))
        return buf

    def render_aov_ids_stripes_device(self, cam, params, rows_per_block, rank, n_ranks, d_buf_ptr, sample_first=0, sample_count=-1, stream=0):
        """Asynchronous: d_buf_ptr is a device pointer to aov_ids_bytes(rows x W) bytes, 16-byte aligned."""
        _check(_hip.hrt_render_aov_ids_stripes_device(self._h, C.byref(cam), C.byref(params), rows_per_block, rank, n_ranks, _vp(d_buf_ptr),
                                                      sample_first, sample_count, _vp(stream)))

    def stats(self):
        st = Stats()
        _check(_hip.hrt_scene_stats(self._h, C.byref(st)))
        return st

    def resolve_u8(self, rgb_linear):
        a = _f32(rgb_linear)
        out = np.empty(a.shape, dtype=np.uint8)
        _check(_hip.hrt_resolve_u8(self._h, _ptr(a), a.size // 3, _ptr(out, _u8p)))
        return out

    def resolve_u8_device(self, d_in_ptr, n_pixels, d_out_ptr, stream=0):
        _check(_hip.hrt_resolve_u8_device(self._h, _vp(d_in_ptr), n_pixels, _vp(d_out_ptr), _vp(stream)))

    def closest_hit(self, params, origins, dirs, t_min=0.001, t_max=float("inf"), pixel0=0):
        o = _f32(origins)
        d = _f32(dirs)
        n = o.shape[0]
        out = np.zeros(n, dtype=HIT_DTYPE)
        _check(_hip.hrt_closest_hit(self._h, C.byref(params), n, _ptr(o), _ptr(d), t_min, t_max, pixel0,
                                    out.ctypes.data_as(C.POINTER(Hit))))
        return out


class MultiScene:
    """hrt_multi_*: the flat scene on several devices of this process + the RCCL gather of their film stripes."""

    def __init__(self, flat, devices=(0,), force_rccl=False, loopback=False):
        """loopback: the test mode of hrt_multi_create (force_rccl < 0) -- a device may be listed once per logical rank and the
        gather is one device copy per rank instead of ncclAllGather."""
        flat_ptr = flat if not isinstance(flat, FlatScene) else C.pointer(flat)
        devs = (C.c_int32 * len(devices))(*devices)
        h = _vp()
        _check(_hip.hrt_multi_create(flat_ptr, len(devices), devs, -1 if loopback else (1 if force_rccl else 0), C.byref(h)))
        self._h = h
        self._keep = flat

    def close(self):
        if getattr(self, "_h", None):
            _hip.hrt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_roulette(self, first_bounce=ROULETTE_FIRST_BOUNCE, q_floor=ROULETTE_Q_FLOOR):
        """DeviceScene.set_roulette for every device of the session (hrt_multi_set_roulette)."""
        _check(_hip.hrt_multi_set_roulette(self._h, first_bounce, q_floor))

    def set_filter(self, kind="mitchell", radius=0.0):
        """DeviceScene.set_filter for every device of the session (hrt_multi_set_filter)."""
        _check(_hip.hrt_multi_set_filter(self._h, _filter_kind(kind), radius))

    def filter_ms(self):
        ms = C.c_double(0.0)
        _check(_hip.hrt_multi_filter_ms(self._h, C.byref(ms)))
        return ms.value

    def progress(self):
        d, t = C.c_uint64(0), C.c_uint64(0)
        _hip.hrt_multi_progress.argtypes = [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _check(_hip.hrt_multi_progress(self._h, C.byref(d), C.byref(t)))
        return d.value, t.value

    @property
    def uses_rccl(self):
        return bool(_hip.hrt_multi_uses_rccl(self._h))

    def render(self, cam, params, rows_per_block=8, sample_first=0, sample_count=-1, resume_sums=None, want_u8=True):
        """-> (sums or means [H, W, 3] float32, u8 film [H, W, 3] or None, Stats)"""
        sums = np.empty((params.height, params.width, 3), dtype=np.float32)
        u8 = np.empty((params.height, params.width, 3), dtype=np.uint8) if want_u8 else None
        rs = None if resume_sums is None else _f32(resume_sums)
        st = Stats()
        _check(_hip.hrt_multi_render(self._h, C.byref(cam), C.byref(params), rows_per_block, sample_first, sample_count,
                                     _ptr(rs) if rs is not None else None, _ptr(sums), _ptr(u8, _u8p) if want_u8 else None, C.byref(st)))
        return sums, u8, st


def math_probe(op, a, b=None, device=0):
    a = _f32(a)
    if op == 5:
        n = a.size // 4
        out = np.empty(n * 4, dtype=np.float32)
    else:
        n = a.size
        out = np.empty(n, dtype=np.float32)
    bb = _f32(b) if b is not None else None
    _check(_hip.hrt_math_probe(device, op, n, _ptr(a), _ptr(bb) if bb is not None else None, _ptr(out)))
    return out


def sampler_probe(seed, keys, device=0):
    """FLAG_STRATIFIED's draw on the GPU: keys uint32 [n, 4] = pixel, sample, bounce, purpose | aux << 8 -> uint32 [n, 4] (the words x, y, z, w)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 4)
    out = np.empty_like(keys)
    u32p = C.POINTER(C.c_uint32)
    _check(_hip.hrt_sampler_probe(device, seed, len(keys), keys.ctypes.data_as(u32p), out.ctypes.data_as(u32p)))
    return out


def debug_bounds_violations(device=0):
    """The 8 violation counters of a -DHRT_DEBUG_BOUNDS build (read and cleared), or None from a normal build."""
    out = (C.c_int64 * 8)()
    _hip.hrt_debug_bounds_violations.argtypes = [C.c_int32, C.POINTER(C.c_int64)]
    st = _hip.hrt_debug_bounds_violations(device, out)
    if st == HRT_ERR_UNSUPPORTED:
        return None
    _check(st)
    return list(out)


def version():
    return _hip.hrt_version().decode()
