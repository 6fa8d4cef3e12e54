"""Build-time guard on the kernels of HRT_FLAG_STRATIFIED, from hipcc's own resource report (no GPU needed), read as
tests/test_nee_resources.py reads it.  The stratified kernels are k_wf_gen_st / k_wf_shade_st / k_wf_shadow_st, one per instantiation
of the kernel each is the twin of, and they keep their twins' budgets: every k_wf_shade_st<false, ...> <= 128 VGPRs (4 waves per SIMD)
and no scratch, its counters variant <= 128 VGPRs and no more scratch than k_wf_shade<true, ...> with the same flags; every
k_wf_shadow_st <= 168 VGPRs, no scratch, three blocks per CU by LDS; k_wf_gen_st no scratch (its counters variant no more than its twin).  The figures are printed: DESIGN.md 4.9
quotes them."""
import pytest

from tests.test_nee_resources import usage  # noqa: F401  (the module-scoped fixture: one hipcc run)

# (NEE, ENV, EMIT, LOBES) of every k_wf_shade the host launches, and (ENV, EMIT, LOBES) of every k_wf_shadow
SHADE = [(0, 0, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (1, 1, 1, 0), (1, 0, 0, 1), (1, 1, 0, 1), (1, 0, 1, 1), (1, 1, 1, 1)]
SHADOW = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


def _find(usage, frag):  # noqa: F811
    hits = {k: v for k, v in usage.items() if frag in k}
    assert hits, f"no {frag} in the report"
    return hits


def _args(stats, flags):
    return "".join(f"Lb{int(b)}E" for b in (stats,) + tuple(flags))


@pytest.mark.parametrize("flags", SHADE)
def test_stratified_shade_variants_keep_their_twins_budget(usage, flags):  # noqa: F811
    for name, u in _find(usage, f"13k_wf_shade_stI{_args(0, flags)}E").items():
        print(f"k_wf_shade_st<false, {flags}>: {u}; twin {list(_find(usage, f'10k_wf_shadeI{_args(0, flags)}E').values())}")
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 128, (name, u)
    twin = max(u["ScratchSize"] for u in _find(usage, f"10k_wf_shadeI{_args(1, flags)}E").values())
    for name, u in _find(usage, f"13k_wf_shade_stI{_args(1, flags)}E").items():
        print(f"k_wf_shade_st<true, {flags}>: {u}; twin's scratch {twin}")
        assert u["VGPRs"] <= 128 and u["ScratchSize"] <= twin, (name, u, twin)


@pytest.mark.parametrize("flags", SHADOW)
def test_stratified_shadow_kernels_keep_their_residency(usage, flags):  # noqa: F811
    for name, u in _find(usage, f"14k_wf_shadow_stI{_args(flags[0], flags[1:])}E").items():
        print(f"k_wf_shadow_st<{flags}>: {u}; twin {list(_find(usage, f'11k_wf_shadowI{_args(flags[0], flags[1:])}E').values())}")
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 168, (name, u)
        assert 3 * u["LDS"] <= 160 * 1024, (name, u)


def test_stratified_gen_kernel_does_not_spill(usage):  # noqa: F811
    for name, u in _find(usage, "11k_wf_gen_stILb0EE").items():
        print(f"k_wf_gen_st<false>: {u}")
        assert u["ScratchSize"] == 0, (name, u)
    twin = max(u["ScratchSize"] for u in _find(usage, "8k_wf_genILb1EE").values())     # (a stack object of the counters kernel, not a spill)
    for name, u in _find(usage, "11k_wf_gen_stILb1EE").items():
        print(f"k_wf_gen_st<true>: {u}; twin's scratch {twin}")
        assert u["ScratchSize"] <= twin, (name, u, twin)


def test_the_default_kernels_keep_their_names(usage):  # noqa: F811
    # the stratified kernels are kernels of their own: every instantiation the other flags launch is still there under its old name
    for flags in SHADE:
        for stats in (0, 1):
            _find(usage, f"10k_wf_shadeI{_args(stats, flags)}E")
    for flags in SHADOW:
        _find(usage, f"11k_wf_shadowI{_args(flags[0], flags[1:])}E")
    for frag in ("8k_wf_genILb0EE", "8k_wf_genILb1EE"):
        _find(usage, frag)
