"""HRT_FLAG_ROULETTE's rule without a GPU: csrc/hrt_roulette.h compiled for the host (tests/tools/roulette_on_cpu.cpp).
The survivor count over all 2^24 values of u is exact -- ceil(q 2^24) -- so the bias of the survival probability is at most 2^-24 / q of
it; a survivor's attenuation is numpy's fp32 quotient bit for bit; attenuations that are not finite or not below 1 are left alone; the
rule draws with a purpose of its own that no other draw uses; and the flag, the setters and the CLI switches are where hrt.h says."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import f64_reference as F
from tests import stratified_np as SN

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F3 = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
RNG_ROULETTE = 8

ATTENS = [(0.5, 0.5, 0.5), (0.73, 0.12, 0.09), (0.1, 0.2, 0.9999999), (1e-3, 2e-3, 5e-4), (0.65, 0.05, 0.05), (0.3333333, 0.1, 0.0),
          (5.9604645e-8, 0.0, 0.0), (0.0, 0.0, 0.0), (0.12, 0.45, 0.14), (2.0 ** -24 * 3, 1e-9, 0.0)]
FLOORS = [0.05, 2.0 ** -20, 0.5, 0.123456]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("roulette") / "libroulettecpu.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-shared", "-o", so,
                           os.path.join(HERE, "tools", "roulette_on_cpu.cpp")])
    L = C.CDLL(so)
    L.roulette_q_c.argtypes = [F3, C.c_float]; L.roulette_q_c.restype = C.c_float
    L.roulette_sweep.argtypes = [F3, C.c_float, C.POINTER(C.c_int64), F3]; L.roulette_sweep.restype = C.c_int
    L.roulette_rule.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_float, F3, C.c_int]
    L.roulette_rule.restype = C.c_int
    L.roulette_constants.argtypes = [np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS"), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    return L


def q_of(atten, floor):
    """the rule's q, restated: fp32 max / min have no rounding"""
    a = np.asarray(atten, np.float32)
    return max(np.float32(min(np.float32(1.0), a.max())), np.float32(floor))


def test_survivor_count_is_exact_and_the_quotient_is_numpys(lib):
    checked = 0
    for atten in ATTENS:
        for floor in FLOORS:
            a = np.array(atten, np.float32)
            q = q_of(a, floor)
            assert q < 1.0
            assert np.float32(lib.roulette_q_c(a, floor)) == q, (atten, floor)
            n, out = C.c_int64(0), np.zeros(3, np.float32)
            same = lib.roulette_sweep(a, floor, C.byref(n), out)
            want = int(np.ceil(float(q) * 2.0 ** 24))          # q 2^24 is exact in float64: #{k : k 2^-24 < q}
            assert n.value == want, (atten, floor, n.value, want)
            assert abs(n.value * 2.0 ** -24 - float(q)) <= 2.0 ** -24          # bias of the survival probability <= 2^-24, i.e. 2^-24 / q of q
            assert same == 1, (atten, floor)
            with np.errstate(all="ignore"):
                assert np.array_equal(out.view(np.uint32), (a / q).view(np.uint32)), (atten, floor, out, a / q)
            checked += 1
    assert checked == len(ATTENS) * len(FLOORS)


@pytest.mark.parametrize("atten", [(1.0, 0.2, 0.2), (0.3, 1.5, 0.1), (0.2, 0.2, 7.0), (np.nan, 0.1, 0.1), (0.1, np.nan, 0.1), (0.1, 0.1, np.nan),
                                   (np.inf, 0.1, 0.1), (0.1, -np.inf, 0.2), (np.inf, np.nan, 0.0), (3e38, 3e38, 3e38)])
def test_full_throughput_nan_and_inf_are_left_alone(lib, atten):
    a = np.array(atten, np.float32)
    assert lib.roulette_q_c(a, 0.05) == 1.0
    n, out = C.c_int64(0), np.zeros(3, np.float32)
    assert lib.roulette_sweep(a, 0.05, C.byref(n), out) == 1
    assert n.value == 1 << 24 and np.array_equal(out.view(np.uint32), a.view(np.uint32))
    for strat in (0, 1):
        b = a.copy()
        assert lib.roulette_rule(1, 2, 3, 4, 5, 0, 0.05, b, strat) == 0 and np.array_equal(b.view(np.uint32), a.view(np.uint32))


def test_a_floor_of_one_switches_the_rule_off(lib):
    a = np.array((0.01, 0.02, 0.03), np.float32)
    assert lib.roulette_q_c(a, 1.0) == 1.0


@pytest.mark.parametrize("strat", [0, 1])
def test_the_rule_draws_word_x_of_its_own_site_and_first_bounce_gates_by_round_plus_one(lib, strat):
    rng = np.random.default_rng(31 + strat)
    seed_lo, seed_hi = 0x89ABCDEF, 0x1234567
    draw = SN.draw if strat else F.draw
    killed = played = 0
    for _ in range(4000):
        pixel, sample = int(rng.integers(0, 1 << 22)), int(rng.integers(0, 4096))
        rnd, first = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        a = rng.random(3).astype(np.float32) * np.float32(0.9)
        q = q_of(a, 0.05)
        b = a.copy()
        got = lib.roulette_rule(seed_lo, seed_hi, pixel, sample, rnd, first, 0.05, b, strat)
        if rnd + 1 < first:                                  # not yet: nothing happens, whatever the coin says
            assert got == 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            continue
        played += 1
        u = F.u01(draw(seed_lo, seed_hi, pixel, sample, rnd, RNG_ROULETTE)[0])
        assert got == int(u >= float(q)), (pixel, sample, rnd, first, a, u, q)
        killed += got
        want = a if got else a / q
        assert np.array_equal(b.view(np.uint32), want.view(np.uint32))
    assert played > 1500 and 0.2 * played < killed < 0.9 * played


def test_the_purposes_keep_their_numbers_and_roulette_is_the_next_free_one(lib):
    p, fb, qf = np.zeros(9, np.uint32), C.c_int32(0), C.c_float(0)
    lib.roulette_constants(p, C.byref(fb), C.byref(qf))
    assert list(p) == [0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert [F.RNG_JITTER, F.RNG_SCATTER, F.RNG_MEDIUM, F.RNG_BALL, F.RNG_BUILD, F.RNG_LENS] == [0, 1, 2, 3, 4, 5]
    assert fb.value == 3 and np.float32(qf.value) == np.float32(0.05)


def _code(path):
    """a source file without its // comments"""
    with open(path) as f:
        return "\n".join(line.split("//")[0] for line in f.read().splitlines())


def test_the_default_render_makes_no_roulette_draw():
    """RNG_ROULETTE is named in two files only: hrt_rng.h, which numbers it, and hrt_roulette.h, whose rule is the one place that draws
    with it.  (That the film without the flag is the one it was is tests/test_gpu_roulette.py's test_off_is_off.)"""
    csrc = os.path.join(ROOT, "hobbyraytracer_amd", "csrc")
    users = [n for n in sorted(os.listdir(csrc)) if "RNG_ROULETTE" in _code(os.path.join(csrc, n))]
    assert users == ["hrt_rng.h", "hrt_roulette.h"], users
    assert _code(os.path.join(csrc, "hrt_rng.h")).count("RNG_ROULETTE") == 1          # the enumerator, no draw


def test_flag_symbols_and_default_params(built):
    from hobbyraytracer_amd import api
    with open(os.path.join(ROOT, "include", "hrt.h")) as f:
        assert re.search(r"HRT_FLAG_ROULETTE = 1u << 10\b", f.read())
    assert api.FLAG_ROULETTE == 1 << 10
    lib = C.CDLL(api.HIP_LIB_PATH)
    for name in ("hrt_scene_set_roulette", "hrt_multi_set_roulette"):
        assert hasattr(lib, name) and name in api.HIP_SYMBOLS
    assert hasattr(api.DeviceScene, "set_roulette") and hasattr(api.MultiScene, "set_roulette")
    off, on = api.default_params(8, 8, 1), api.default_params(8, 8, 1, roulette=True)
    assert off.flags & api.FLAG_ROULETTE == 0 and on.flags == off.flags | (1 << 10)
    both = api.default_params(8, 8, 1, roulette=True, nee=True, stratified=True)
    assert both.flags == api.FLAG_ROULETTE | api.FLAG_NEE | api.FLAG_STRATIFIED
    assert C.sizeof(api.Params) == 36                          # hrt_params did not grow


@pytest.mark.parametrize("setter", ["hrt_scene_set_roulette", "hrt_multi_set_roulette"])
def test_the_setters_reject_invalid_values(built, setter):
    """the values are judged before the handle, so this needs no device: a NULL handle with valid values says "NULL", with invalid ones
    names the value"""
    from hobbyraytracer_amd import api
    f = getattr(api._hip, setter)
    for first, floor, word in [(-1, 0.05, "first_bounce"), (-2 ** 31, 0.5, "first_bounce"), (3, 0.0, "q_floor"), (3, -0.1, "q_floor"),
                               (3, 1.0000001, "q_floor"), (3, float("nan"), "q_floor"), (3, float("inf"), "q_floor"), (0, -0.0, "q_floor")]:
        assert f(None, first, floor) == api.HRT_ERR_INVALID
        assert word in api._hip.hrt_last_error().decode(), (first, floor)
    for first, floor in [(0, 1.0), (3, 0.05), (2 ** 31 - 1, 1e-30)]:
        assert f(None, first, floor) == api.HRT_ERR_INVALID
        assert "NULL" in api._hip.hrt_last_error().decode()


@pytest.mark.parametrize("flags, message", [
    (["--roulette-floor", "0"], "--roulette-floor"),
    (["--roulette-floor", "1.5"], "--roulette-floor"),
    (["--roulette-floor", "nan"], "--roulette-floor"),
    (["--roulette-floor", "abc"], "--roulette-floor"),
    (["--roulette-floor", "-0.2"], "--roulette-floor"),
    (["--roulette-start", "-1"], "--roulette-start"),
    (["--roulette-start", "two"], "--roulette-start"),
    (["--roulette-start", "3.5"], "--roulette-start"),
    (["--roulette", "--roulette-start"], "--roulette-start"),
])
def test_cli_refuses_bad_roulette_values(built, scenes_dir, tmp_path, flags, message):
    from hobbyraytracer_amd import api
    r = subprocess.run([api.CLI_PATH, os.path.join(scenes_dir, "cornell_box.yaml"), "--size", "16x16"] + flags, cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stdout + r.stderr
    err = r.stderr.strip().splitlines()
    assert len(err) == 1 and message in err[0], r.stderr
    assert "Loaded scene" not in r.stdout            # refused before the scene (and any device) is touched


@pytest.mark.parametrize("flags", [["--roulette"], ["--roulette-start", "0"], ["--roulette-floor", "0.25"], ["--roulette-floor", "1"],
                                   ["--roulette", "--roulette-start", "5", "--roulette-floor", "0.1", "--nee", "--stratified"]])
def test_cli_accepts_the_three_switches(built, scenes_dir, tmp_path, flags):
    """parsing only: the scene loads; what follows needs a device (tests/test_gpu_roulette.py renders with them)"""
    from hobbyraytracer_amd import api
    r = subprocess.run([api.CLI_PATH, os.path.join(scenes_dir, "cornell_box.yaml"), "--size", "16x16", "--spp", "1", "--no-progress"] + flags,
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode != 2 and "Loaded scene" in r.stdout, r.stdout + r.stderr
    with open(os.path.join(ROOT, "hobbyraytracer_amd", "host", "main.cpp")) as f:
        usage = f.read().split("#include")[0]
    for switch in ("--roulette ", "--roulette-start N", "--roulette-floor Q"):
        assert switch in usage
