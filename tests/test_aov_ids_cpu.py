"""Id mattes and position (hrt_render_aov_ids_*) without a GPU: the entry points are declared in include/hrt.h,
exported by libhrt_hip.so and bound by hobbyraytracer_amd/api.py; the header is still C99; hrt_aov_ids_bytes answers; the CLI refuses
--aov-ids without --aov and a malformed --matte with exit 2; NULL arguments are refused before any device is touched; and the numpy
restatement of the matte rule (tests/aov_ids_np.py) has the properties the header states."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import aov_ids_np as ref
from tests.test_abi import ROOT, _declared_functions

SYMBOLS = ("hrt_aov_ids_bytes", "hrt_render_aov_ids_tile", "hrt_render_aov_ids_stripes_device", "hrt_render_aov_ids_stripes")


def test_the_symbols_are_declared_exported_and_bound(built):
    from hobbyraytracer_amd import api
    declared = _declared_functions("hrt.h")
    lib = C.CDLL(api.HIP_LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, f"include/hrt.h does not declare {name}"
        assert hasattr(lib, name), f"libhrt_hip.so does not export {name}"
        assert name in api.HIP_SYMBOLS
    for method in ("render_aov_ids_tile", "render_aov_ids_stripes", "render_aov_ids_stripes_device"):
        assert callable(getattr(api.DeviceScene, method))
    assert callable(api.split_aov_ids) and callable(api.matte)
    assert not hasattr(lib, "hrt_aov_ids_launch")            # the bridge between the two translation units is not part of the ABI
    assert (api.AOV_ID_SLOTS, api.AOV_ID_RANKS, api.AOV_ID_UNUSED) == (ref.SLOTS, ref.RANKS, ref.UNUSED)


def test_the_header_is_still_c99_and_declares_the_documented_signatures(built, tmp_path):
    src = tmp_path / "ids.c"
    src.write_text(f'#include "{ROOT}/include/hrt.h"\n'
                   "uint64_t (*z)(int64_t) = hrt_aov_ids_bytes;\n"
                   "hrt_status (*a)(hrt_scene*, const hrt_camera*, const hrt_params*, hrt_rect, void*) = hrt_render_aov_ids_tile;\n"
                   "hrt_status (*b)(hrt_scene*, const hrt_camera*, const hrt_params*, int32_t, int32_t, int32_t, void*, int32_t, int32_t, void*) = "
                   "hrt_render_aov_ids_stripes_device;\n"
                   "hrt_status (*c)(hrt_scene*, const hrt_camera*, const hrt_params*, int32_t, int32_t, int32_t, void*, int32_t, int32_t) = "
                   "hrt_render_aov_ids_stripes;\n"
                   "typedef char slots[HRT_AOV_ID_SLOTS == 8 ? 1 : -1];\ntypedef char ranks[HRT_AOV_ID_RANKS == 4 ? 1 : -1];\n"
                   "int main(void){ return z && a && b && c ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-o", str(tmp_path / "ids.o"), str(src)])


def test_ids_bytes(built):
    from hobbyraytracer_amd import api
    assert api.AOV_IDS_DTYPE.itemsize == 80
    for n, want in ((0, 0), (1, 80), (24 * 16, 24 * 16 * 80), (2 ** 30, 80 * 2 ** 30), (-1, 0), (-2 ** 40, 0)):
        assert api.aov_ids_bytes(n) == want, n


def test_null_arguments_are_refused_before_any_device_is_touched(built):
    from hobbyraytracer_amd import api
    cam, p = api.Camera(), api.default_params(8, 8, 1)
    out = np.full(8 * 8 * 20, 7.0, np.float32)
    ptr = C.c_void_p(out.ctypes.data)
    assert api._hip.hrt_render_aov_ids_tile(None, C.byref(cam), C.byref(p), api.Rect(0, 0, 8, 8), ptr) == api.HRT_ERR_INVALID
    assert b"NULL" in api._hip.hrt_last_error()
    assert api._hip.hrt_render_aov_ids_stripes(None, C.byref(cam), C.byref(p), 4, 0, 1, ptr, 0, -1) == api.HRT_ERR_INVALID
    assert api._hip.hrt_render_aov_ids_stripes_device(None, C.byref(cam), C.byref(p), 4, 0, 1, ptr, 0, -1, None) == api.HRT_ERR_INVALID
    assert (out == 7.0).all()


@pytest.mark.parametrize("args, word", [
    (("--aov-ids",), "--aov"),
    (("--matte", "object:1", "m.pfm"), "--aov"),                       # --matte implies --aov-ids, which needs --aov
    (("--aov", "p", "--matte", "1,2", "m.pfm"), "--matte"),            # no kind
    (("--aov", "p", "--matte", "triangle:1", "m.pfm"), "--matte"),     # a kind that is not reported
    (("--aov", "p", "--matte", "object:", "m.pfm"), "--matte"),        # no id
    (("--aov", "p", "--matte", "object:1,", "m.pfm"), "--matte"),
    (("--aov", "p", "--matte", "material:1,x", "m.pfm"), "--matte"),
    (("--aov", "p", "--matte", "object:16777216", "m.pfm"), "--matte"),   # 2^24: not an id a PFM file can carry
    (("--aov", "p", "--matte", "object:-2", "m.pfm"), "--matte"),
    (("--aov", "p", "--matte", "object:1"), "--matte"),                # no file
])
def test_cli_usage_errors(built, tmp_path, args, word):
    from hobbyraytracer_amd import api
    r = subprocess.run([api.CLI_PATH, "no_such_scene.yaml", *args], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (args, r.returncode, r.stdout, r.stderr)
    assert word in r.stderr, (args, r.stderr)
    assert not list(tmp_path.iterdir())


# ---- the restatement's properties ----
def _one(ids):
    return ref.ranks(np.asarray(ids))


@pytest.mark.parametrize("S", [1, 2, 4, 16, 64, 256])
def test_at_most_four_ids_cover_exactly_one_for_power_of_two_counts(S):
    r = np.random.default_rng(S)
    for distinct in (1, 2, 3, 4):
        for _ in range(20):
            ids = r.choice(r.choice(np.arange(-1, 50), distinct, replace=False), S)
            oid, cov = _one(ids)
            used = oid != ref.UNUSED
            assert used.sum() == len(set(ids.tolist())) <= distinct
            # every count / S is exact for a power of two S, and so is every partial sum of them: the sum is 1 in any order
            assert cov.dtype == np.float32 and np.float32(cov[0] + cov[1] + cov[2] + cov[3]) == np.float32(1)
            assert (np.diff(cov) <= 0).all()


def test_tie_order_is_by_id_ascending_signed():
    oid, cov = _one([5, 3, 5, 3, -1, 9, -1, 9])
    assert oid.tolist() == [-1, 3, 5, 9] and cov.tolist() == [0.25] * 4
    oid, cov = _one([7, 7, 7, 2, 2, 4, 4, 1])                   # the count comes first, then the id
    assert oid.tolist() == [7, 2, 4, 1] and cov.tolist() == [0.375, 0.25, 0.25, 0.125]
    oid, _ = _one([2 ** 24 - 1, 0, -1])
    assert oid.tolist() == [-1, 0, 2 ** 24 - 1, ref.UNUSED]


def test_first_seen_eviction_with_nine_or_more_ids():
    # ids 0 .. 7 fill the table; 8 and 9 are dropped however often they come, and what they would have covered is missing from the sum
    ids = list(range(8)) + [8] * 5 + [9] * 2 + [7]
    assert ref.table(ids) == [(k, 1) for k in range(7)] + [(7, 2)]
    oid, cov = _one(ids)
    assert oid.tolist() == [7, 0, 1, 2]
    assert cov.tolist() == [np.float32(2) / np.float32(16)] + [np.float32(1) / np.float32(16)] * 3
    # the table keeps who came first, not who is largest: the late majority is not reported at all
    oid, cov = _one(list(range(10, 18)) + [3] * 56)
    assert 3 not in oid.tolist() and oid.tolist() == [10, 11, 12, 13] and float(cov.sum()) == 4 / 64
    # ... but an id that is in the table keeps counting after the table is full
    oid, cov = _one(list(range(10, 18)) + [99, 17, 17, 98])
    assert oid[0] == 17 and cov[0] == np.float32(3) / np.float32(12)


def test_unused_ranks():
    oid, cov = _one([4, 4, 4])
    assert oid.tolist() == [4, ref.UNUSED, ref.UNUSED, ref.UNUSED]
    assert cov.view(np.uint32).tolist() == [np.float32(1).view(np.uint32), 0, 0, 0]        # +0, not -0
    oid, cov = _one([-1])
    assert oid.tolist() == [-1, ref.UNUSED, ref.UNUSED, ref.UNUSED] and cov[0] == 1


def test_position_is_the_sum_in_sample_order_divided_once():
    r = np.random.default_rng(3)
    pos = (r.standard_normal((7, 2, 3, 3)) * 1e3).astype(np.float32)
    got = ref.mean_position(pos)
    want = np.zeros((2, 3, 3), np.float32)
    for s in range(7):
        want = (want + pos[s]).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), (want / np.float32(7)).view(np.uint32))
    one = np.array([[[-0.0, 1.5, -2.0]]], np.float32)            # (+0 + -0) / 1 = +0
    assert ref.mean_position(one).view(np.uint32).tolist() == [[0, np.float32(1.5).view(np.uint32), np.float32(-2).view(np.uint32)]]


def test_matte_of_all_reported_ids_is_the_coverage_sum(built):
    from hobbyraytracer_amd import api
    r = np.random.default_rng(11)
    S, shape = 48, (5, 6)
    obj = r.integers(-1, 12, (S,) + shape)
    mat = r.integers(-1, 3, (S,) + shape)
    out = ref.mattes(obj, mat, np.zeros((S,) + shape + (3,), np.float32))
    for kind, n_ids in (("object", 12), ("material", 3)):
        ids, cov = out[kind + "_id"], out[kind + "_coverage"]
        total = np.zeros(shape, np.float32)
        for k in range(ref.RANKS):
            total = total + cov[..., k]
        everything = list(range(-1, n_ids)) + [ref.UNUSED]
        for fn in (api.matte, ref.matte):
            assert np.array_equal(fn(ids, cov, everything).view(np.uint32), total.view(np.uint32)), (kind, fn)
            assert np.array_equal(fn(ids, cov, [-7]), np.zeros(shape, np.float32))
            parts = fn(ids, cov, [0]).astype(np.float64) + fn(ids, cov, list(range(1, n_ids)) + [-1]).astype(np.float64)
            assert np.allclose(parts, total, atol=1e-6)
        assert np.array_equal(api.matte(ids, cov, [0, 2]).view(np.uint32), ref.matte(ids, cov, [0, 2]).view(np.uint32))
        assert np.array_equal(api.matte(ids, cov, 1), ref.matte(ids, cov, [1]))
    assert (out["material_coverage"].sum(axis=-1) > 0.999).all()          # three materials and the miss: nothing was dropped
    assert (out["object_coverage"].sum(axis=-1) < 1).any()                # thirteen object ids: some pixel dropped samples


def test_split_aov_ids_names_the_five_groups(built):
    from hobbyraytracer_amd import api
    raw = np.arange(2 * 3 * 20, dtype=np.uint32).reshape(2, 3, 20)
    buf = raw.view(api.AOV_IDS_DTYPE).reshape(2, 3)
    d = api.split_aov_ids(buf)
    assert d["position"].shape == (2, 3, 3) and d["position"].dtype == np.float32
    assert d["object_id"].shape == d["material_id"].shape == (2, 3, 4) and d["object_id"].dtype == np.int32
    px = raw[1, 2]
    assert np.array_equal(d["position"][1, 2].view(np.uint32), px[0:3])
    assert np.array_equal(d["object_id"][1, 2].view(np.uint32), px[4:8]) and np.array_equal(d["object_coverage"][1, 2].view(np.uint32), px[8:12])
    assert np.array_equal(d["material_id"][1, 2].view(np.uint32), px[12:16]) and np.array_equal(d["material_coverage"][1, 2].view(np.uint32), px[16:20])
    with pytest.raises(ValueError):
        api.split_aov_ids(raw)
