"""The measured variance (include/hrt.h "measured variance") without a GPU: the C ABI is declared, exported, bound and still
C99; bad arguments are refused before any device is touched with the outputs untouched; the numpy restatement of the header's words
(tests/variance_np.py) is exact where it can be, agrees with the per-sample formula of the adaptive render and estimates a known variance;
and with it the guided denoiser gets closer to a converged film than with its spatial estimate on two scenes -- the quality test, decided
here because GPU films are the oracle's bits and tests/test_gpu_variance.py requires the kernels to give the restatement's bits."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import denoise_np as dn
from tests import variance_np as vn
from tests.test_abi import ROOT, _declared_functions
from tests.test_denoise_cpu import QUALITY_H, QUALITY_SPP, QUALITY_W, REFERENCE_SPP, oracle_feature_buffers, rms

VARIANCE_SYMBOLS = ("hrt_variance_state_bytes", "hrt_variance_fold_device", "hrt_variance_finish_device", "hrt_adaptive_variance_device",
                    "hrt_variance_fold", "hrt_variance_finish", "hrt_adaptive_variance")
MEASURED_SIGMA_L = 6.0          # what the CLI takes under --denoise-variance measured (host/main.cpp kMeasuredSigmaL; the sweep of DESIGN.md 4.13)
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the C ABI
def test_the_symbols_are_declared_exported_and_bound(built):
    from hobbyraytracer_amd import api
    declared = _declared_functions("hrt.h")
    lib = C.CDLL(api.HIP_LIB_PATH)
    for name in VARIANCE_SYMBOLS:
        assert name in declared, f"include/hrt.h does not declare {name}"
        assert hasattr(lib, name), f"libhrt_hip.so does not export {name}"
        assert name in api.HIP_SYMBOLS
    for f in (api.variance_fold, api.variance_finish, api.adaptive_variance, api.variance_fold_device, api.variance_finish_device,
              api.adaptive_variance_device, api.variance_state_bytes, api.variance_batches, api.DeviceScene.render_stripes_with_variance):
        assert callable(f)
    assert api.variance_state_bytes(640 * 640) == 8 * 640 * 640
    assert api.variance_state_bytes(0) == 0 and api.variance_state_bytes((1 << 30) + 1) == 0 and api.variance_state_bytes(1 << 30) == 8 << 30
    assert api.variance_batches(8, 3) == vn.batch_ranges(8, 3) == [(0, 3), (3, 3), (6, 2)]
    assert api.variance_batches(9, 4) == vn.batch_ranges(9, 4) == [(0, 3), (3, 3), (6, 3)]
    assert api.variance_batches(16, 4) == [(0, 4), (4, 4), (8, 4), (12, 4)] and api.variance_batches(3, 64) == [(0, 1), (1, 1), (2, 1)]
    main_cpp = open(f"{ROOT}/hobbyraytracer_amd/host/main.cpp").read()
    assert f"kMeasuredSigmaL = {MEASURED_SIGMA_L:.1f}f" in main_cpp          # the quality test below decides on the CLI's value


def test_the_header_is_c99_with_the_entry_points_types(built, tmp_path):
    from hobbyraytracer_amd import api
    src = tmp_path / "var.c"
    src.write_text(f'#include "{ROOT}/include/hrt.h"\n'
                   "uint64_t (*a)(int64_t) = hrt_variance_state_bytes;\n"
                   "hrt_status (*b)(int, int64_t, const float*, float, int32_t, int32_t, float*, void*) = hrt_variance_fold_device;\n"
                   "hrt_status (*c)(int, int64_t, const float*, int32_t, int32_t, float*, void*) = hrt_variance_finish_device;\n"
                   "hrt_status (*d)(int, int64_t, const float*, const float*, const int32_t*, float*, void*) = hrt_adaptive_variance_device;\n"
                   "hrt_status (*e)(int, int64_t, const float*, float, int32_t, int32_t, float*) = hrt_variance_fold;\n"
                   "hrt_status (*f)(int, int64_t, const float*, int32_t, int32_t, float*) = hrt_variance_finish;\n"
                   "hrt_status (*g)(int, int64_t, const float*, const float*, const int32_t*, float*) = hrt_adaptive_variance;\n"
                   "int main(void){ return a && b && c && d && e && f && g && a(3) == 24 ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-o", str(tmp_path / "var.o"), str(src)])
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "var"), str(src), "-L" + api.LIB_DIR, "-lhrt_hip", "-Wl,-rpath," + api.LIB_DIR,
                           "-Wl,-rpath,/opt/rocm/lib"])
    subprocess.check_call([str(tmp_path / "var")])


def test_bad_arguments_are_refused_before_any_device_is_touched_and_leave_the_outputs_untouched(built):
    from hobbyraytracer_amd import api
    n = 12
    rgb, sq = np.ones((n, 3), np.float32), np.ones(n, np.float32)
    count = np.full(n, 4, np.int32)
    state, var = np.full((n, 2), 7.0, np.float32), np.full(n, 7.0, np.float32)
    assert state.ctypes.data % 8 == 0
    hip = api._hip
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a)      # noqa: E731
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731

    def fold(dev, n=n, r=rgb, scale=1.0, done=4, c=4, s=state):
        if dev:
            return hip.hrt_variance_fold_device(0, n, vp(r), scale, done, c, vp(s), None)
        return hip.hrt_variance_fold(0, n, fp(r), scale, done, c, fp(s))

    def finish(dev, n=n, s=state, samples=8, batches=2, v=var):
        if dev:
            return hip.hrt_variance_finish_device(0, n, vp(s), samples, batches, vp(v), None)
        return hip.hrt_variance_finish(0, n, fp(s), samples, batches, fp(v))

    def adaptive(dev, n=n, su=rgb, q=sq, k=count, v=var):
        if dev:
            return hip.hrt_adaptive_variance_device(0, n, vp(su), vp(q), vp(k), vp(v), None)
        return hip.hrt_adaptive_variance(0, n, fp(su), fp(q), ip(k), fp(v))

    def refused(st, word):
        assert st == api.HRT_ERR_INVALID, (st, word)
        assert word.encode() in hip.hrt_last_error(), (word, hip.hrt_last_error())
        assert (state == 7.0).all() and (var == 7.0).all()

    for dev in (False, True):
        for call, args in ((fold, ("r", "s")), (finish, ("s", "v")), (adaptive, ("su", "q", "k", "v"))):
            for missing in args:
                refused(call(dev, **{missing: None}), "NULL")
            refused(call(dev, n=0), "n_pixels")
            refused(call(dev, n=-5), "n_pixels")
            refused(call(dev, n=(1 << 30) + 1), "2^30")
        refused(fold(dev, done=-1), "samples_before")
        refused(fold(dev, c=0), "samples_batch")
        refused(fold(dev, c=-3), "samples_batch")
        refused(fold(dev, done=0x7fffffff, c=1), "samples_before + samples_batch")
        for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
            refused(fold(dev, scale=bad), "scale")
        refused(finish(dev, batches=1), "batches")
        refused(finish(dev, batches=0), "batches")
        refused(finish(dev, samples=3, batches=4), "samples")
    refused(hip.hrt_variance_fold_device(0, n - 1, vp(rgb), 1.0, 4, 4, C.c_void_p(state.ctypes.data + 4), None), "misaligned")
    refused(hip.hrt_variance_fold_device(0, n - 1, C.c_void_p(rgb.ctypes.data + 2), 1.0, 4, 4, vp(state), None), "misaligned")
    refused(hip.hrt_variance_finish_device(0, n - 1, C.c_void_p(state.ctypes.data + 4), 8, 2, vp(var), None), "misaligned")
    refused(hip.hrt_adaptive_variance_device(0, n - 1, vp(rgb), C.c_void_p(sq.ctypes.data + 1), vp(count), vp(var), None), "misaligned")
    # the Python wrappers check the shapes themselves
    with pytest.raises(ValueError):
        api.variance_fold(rgb[:, :2], 0, 4)
    with pytest.raises(ValueError):
        api.variance_fold(rgb, 4, 4)                       # a continuation without a state
    with pytest.raises(ValueError):
        api.variance_fold(rgb, 4, 4, state[:5])
    with pytest.raises(ValueError):
        api.variance_finish(var, 8, 2)
    with pytest.raises(ValueError):
        api.adaptive_variance(rgb, sq[:5], count)
    with pytest.raises(ValueError):
        api.variance_batches(0, 4)


# ---------------------------------------------------------------- properties of the restatement
def test_two_equal_halves_of_dyadic_values_give_the_exact_variance():
    """Batches A and B of 4 samples each, grey pixels whose sums are powers of two (or 0): Y(1, 1, 1) is exactly 1 in fp32, so the
    luminance of such a sum is the sum itself and every operation of the two folds and the finish is exact.  With batch means mA and mB
    the result is then ((mA - mB) / 2)^2 / 1 -- M2 = (mB - mA)^2 * (4 * 4 / 8), over batches - 1 = 1, over 8 samples -- bit for bit."""
    assert dn.lum(F(1), F(1), F(1)) == F(1)
    sum_a = np.array([0.0, 4.0, 4.0, 8.0, 2.0, 16.0, 1.0, 0.0, 0.5], F)         # after batch A
    sum_ab = np.array([4.0, 8.0, 16.0, 16.0, 16.0, 16.0, 32.0, 0.0, 0.5], F)    # after batch B
    grey = lambda v: np.stack([v, v, v], axis=-1)      # noqa: E731
    mA, mB = sum_a.astype(np.float64) / 4, (sum_ab.astype(np.float64) - sum_a) / 4
    exact = ((mA - mB) / 2) ** 2 / 1
    assert len(np.unique(exact)) >= 6
    var = vn.from_batches([grey(sum_a), grey(sum_ab)], [4, 4])
    assert var.dtype == np.float32 and np.array_equal(var.astype(np.float64), exact)
    # ... and the same from the divided final buffer (scale = 8 puts the power of two back exactly)
    var = vn.from_batches([grey(sum_a), grey(sum_ab / F(8))], [4, 4], samples=8)
    assert np.array_equal(var.astype(np.float64), exact)


def _samples(n, pixels, seed, mean=1.0, sigma=0.4):
    """n samples of `pixels` pixels, [n, pixels, 3] fp32, positive, with sigma / mean of the luminance >= 0.1 in every pixel's population"""
    r = np.random.default_rng(seed)
    level = r.uniform(0.5, 2.0, (1, pixels, 3)) * mean
    return np.abs(level * (1.0 + sigma * r.standard_normal((n, pixels, 1)))).astype(F)      # (one draw per sample: the channels move together)


def _running(samples):
    """what the render keeps: sums [j] after sample j (fp32, in sample order), and the adaptive render's sq and count after the last"""
    sums, sq = np.zeros(samples.shape[1:], F), np.zeros(samples.shape[1], F)
    after = []
    for s in samples:
        sums = sums + s
        y = dn.lum(s[..., 0], s[..., 1], s[..., 2])
        sq = sq + y * y
        after.append(sums)
    return after, sq, np.full(samples.shape[1], len(samples), np.int32)


def test_one_sample_per_batch_agrees_with_the_per_sample_formula_of_the_adaptive_render():
    """K = n batches of one sample each estimate what the adaptive render's (sq - n m m) / (n - 1) / n estimates, from the same samples.
    Both against a float64 evaluation of the sample variance of the fp32 luminances: each formula passes its result through at most
    ~n roundings (u = 2^-24 each) of quantities as large as n (mean^2 + sigma^2) while the result is n sigma^2, so the relative error
    fp32 allows is bounded by 4 n u (1 + (mean / sigma)^2) -- the sq side's cancellation; the batch side's is 2 (mean / sigma) of it at
    most --, and the two agree within twice that."""
    n, P = 16, 4000
    samples = _samples(n, P, 7)
    after, sq, count = _running(samples)
    batch = vn.from_batches(after, [1] * n)
    per_sample = dn.variance_of_mean_luminance(after[-1], sq, count)
    assert np.array_equal(_bits(per_sample), _bits(vn.adaptive(after[-1], sq, count)))          # word for word the same formula
    y64 = dn.lum(samples[..., 0], samples[..., 1], samples[..., 2]).astype(np.float64)
    mean64, var64 = y64.mean(axis=0), y64.var(axis=0, ddof=1)
    assert (np.sqrt(var64) / mean64 >= 0.1).all()
    bound = 4 * n * 2.0 ** -24 * (1 + mean64 ** 2 / var64)
    want = var64 / n
    err_b, err_s = np.abs(batch - want) / want, np.abs(per_sample - want) / want
    print(f"\nrelative error, worst pixel: batch means {err_b.max():.3g}, sq - n m m {err_s.max():.3g}, bound there {bound[np.argmax(err_s)]:.3g}")
    assert (err_b <= bound).all() and (err_s <= bound).all()
    assert (np.abs(batch - per_sample) <= 2 * bound * want).all()


def test_the_estimate_of_a_known_gaussian_variance_is_unbiased():
    """10^4 pixels of iid Gaussian noise of known sigma, 16 samples in K = 4 batches: each pixel's estimate of sigma^2 / n has the
    relative standard deviation sqrt(2 / (K - 1)), so the mean of the estimates lies within 4 standard errors, 4 sqrt(2 / (K - 1)) /
    sqrt(pixels) = 3.3 %, of sigma^2 / n (fp32 rounding is five orders below that)."""
    n, K, P, sigma = 16, 4, 10000, 0.2
    r = np.random.default_rng(11)
    v = (1.0 + sigma * r.standard_normal((n, P))).astype(F)
    samples = np.stack([v, v, v], axis=-1)                       # grey: Y(v, v, v) = v within an ulp
    after, _, _ = _running(samples)
    ranges = vn.batch_ranges(n, K)
    var = vn.from_batches([after[first + c - 1] for first, c in ranges], [c for _, c in ranges])
    want = sigma ** 2 / n
    se = want * np.sqrt(2.0 / (K - 1)) / np.sqrt(P)
    got = float(var.astype(np.float64).mean())
    print(f"\nmean estimate {got:.6g}, sigma^2 / n {want:.6g}, {abs(got - want) / se:.2f} standard errors")
    assert abs(got - want) <= 4 * se
    # the spread is the chi-square's: the estimator is what it is said to be, not merely right on average
    rel_sd = float(var.astype(np.float64).std() / want)
    assert abs(rel_sd - np.sqrt(2.0 / (K - 1))) < 0.05


# ---------------------------------------------------------------- quality
QUALITY_BATCH_SEEDS = (11, 12, 13, 14)


def measured_quality_case(api, orc, scenes_dir, assets, scene, seeds=QUALITY_BATCH_SEEDS):
    """-> (accumulation buffers after each batch (undivided fp32 sums), samples per batch, feature buffer, reference film) of one scene.
    The oracle has no sample ranges: batch j is an oracle film of seed seeds[j] with QUALITY_SPP / len(seeds) samples, statistically
    what a sample range is; its sum is film * samples, the feature buffer the mean of the batches' feature buffers."""
    hs = api.HostScene(f"{scenes_dir}/{scene}", assets)
    cam = hs.camera(QUALITY_W, QUALITY_H)
    world = orc.World(hs.flat_ptr)
    c = QUALITY_SPP // len(seeds)
    assert c * len(seeds) == QUALITY_SPP
    sums, after, aov = np.zeros((QUALITY_H, QUALITY_W, 3), F), [], np.zeros((QUALITY_H, QUALITY_W, 8), F)
    for seed in seeds:
        p = api.default_params(QUALITY_W, QUALITY_H, c, seed=seed)
        film, _ = world.render_tile(cam, p)
        sums = sums + film.astype(F) * F(c)
        after.append(sums)
        aov = aov + oracle_feature_buffers(api, orc, hs, world, cam, p)
    aov = aov / F(len(seeds))
    ref, _ = world.render_tile(cam, api.default_params(QUALITY_W, QUALITY_H, REFERENCE_SPP, seed=2))
    return after, c, aov, ref


@pytest.mark.parametrize("scene", ["cornell_box.yaml", "material_zoo.yaml"])
def test_the_measured_variance_beats_the_spatial_estimate_against_a_converged_film(built, assets, scenes_dir, scene):
    """The scenes, size, samples and reference of test_filtering_lowers_the_rms_error_against_a_converged_film; the noisy film is the fp32
    mean of four 4-spp oracle films of different seeds.  Filtered with the batch-means variance of the restatement (K = 4) and the
    sigma_l the CLI takes under --denoise-variance measured, the RMS error is below that of the same film filtered with the spatial
    estimate and the shipped defaults, and below the unfiltered film's."""
    from hobbyraytracer_amd import api
    from oracle import oracle_py as orc
    after, c, aov, ref = measured_quality_case(api, orc, scenes_dir, assets, scene)
    noisy = (after[-1] / F(QUALITY_SPP)).astype(F)
    assert np.isfinite(noisy).all() and np.isfinite(ref).all()
    var = vn.from_batches(after, [c] * len(after))
    before = rms(noisy, ref)
    spatial = rms(dn.denoise(noisy, aov), ref)
    measured = rms(dn.denoise(noisy, aov, var, sigma_l=MEASURED_SIGMA_L), ref)
    print(f"\n{scene}: rms before {before:.5f}, spatial estimate (sigma_l 2.5) {spatial:.5f} (ratio {spatial / before:.4f}), "
          f"measured K = 4 (sigma_l {MEASURED_SIGMA_L:g}) {measured:.5f} (ratio {measured / before:.4f})")
    assert measured < spatial, (scene, measured, spatial)
    assert measured < before, (scene, measured, before)


@pytest.mark.parametrize("flags", [["--denoise-variance", "guessed"], ["--denoise-variance"], ["--denoise-batches", "1"], ["--denoise-batches", "65"],
                                   ["--denoise-batches", "four"], ["--dump-variance", "u.pfm"], ["--denoise", "--dump-variance", "u.pfm"],
                                   ["--denoise-variance", "spatial", "--dump-variance", "u.pfm"]])
def test_cli_usage_errors_exit_2_before_anything_is_loaded(built, scenes_dir, tmp_path, flags):
    from hobbyraytracer_amd import api
    r = subprocess.run([api.CLI_PATH, f"{scenes_dir}/cornell_box.yaml", "--size", "16x16", "--spp", "4", "--no-progress", "--out", "u.png"] + flags,
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and r.stderr.strip(), (flags, r.returncode, r.stdout + r.stderr)
    assert "Loaded scene" not in r.stdout and not list(tmp_path.iterdir())


@pytest.mark.parametrize("flags", [["--denoise-variance", "measured"], ["--denoise-batches", "8", "--dump-variance", "v.pfm"],
                                   ["--denoise-variance", "measured", "--progressive", "2"], ["--denoise-variance", "spatial", "--denoise-batches", "3"]])
def test_cli_accepts_the_switches(built, scenes_dir, tmp_path, flags):
    """parsing only: the scene loads; what follows needs a device (tests/test_gpu_variance.py renders with them)"""
    from hobbyraytracer_amd import api
    r = subprocess.run([api.CLI_PATH, f"{scenes_dir}/cornell_box.yaml", "--size", "16x16", "--spp", "4", "--no-progress"] + flags,
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode != 2 and "Loaded scene" in r.stdout, r.stdout + r.stderr
    usage = open(f"{ROOT}/hobbyraytracer_amd/host/main.cpp").read().split("#include")[0]
    for switch in ("--denoise-variance spatial|measured", "--denoise-batches K", "--dump-variance FILE.pfm"):
        assert switch in usage
