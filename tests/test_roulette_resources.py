"""Build-time guard on the kernels of HRT_FLAG_ROULETTE, from hipcc's own resource report (no GPU needed), read as
tests/test_nee_resources.py reads it.  The roulette kernels are k_wf_shade_rr and k_wf_shade_st_rr, twins of k_wf_shade and k_wf_shade_st
for the nine flag combinations the host launches, without the counters variants (the flag refuses HRT_FLAG_STATS): each keeps the shade
budget of <= 128 VGPRs (4 waves per SIMD) and no scratch.  The figures are printed: DESIGN.md 4.10 quotes them."""
import pytest

from tests.test_nee_resources import usage  # noqa: F401  (the module-scoped fixture: one hipcc run)
from tests.test_stratified_resources import SHADE, SHADOW, _args, _find


@pytest.mark.parametrize("flags", SHADE)
@pytest.mark.parametrize("kernel, twin", [("13k_wf_shade_rr", "10k_wf_shade"), ("16k_wf_shade_st_rr", "13k_wf_shade_st")])
def test_roulette_shade_variants_keep_the_shade_budget(usage, kernel, twin, flags):  # noqa: F811
    hits = _find(usage, f"{kernel}I{_args(0, flags)}E")
    for name, u in hits.items():
        print(f"{kernel[2:]}<false, {flags}>: {u}; twin {list(_find(usage, f'{twin}I{_args(0, flags)}E').values())}")
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 128, (name, u)


def test_there_are_no_counting_variants_and_no_second_copy_of_the_other_kernels(usage):  # noqa: F811
    names = [k for k in usage if "_rr" in k]
    assert len(names) == 2 * len(SHADE), names
    assert all("k_wf_shade_rrILb0E" in k or "k_wf_shade_st_rrILb0E" in k for k in names), names


def test_the_default_and_stratified_kernels_keep_their_names(usage):  # noqa: F811
    # the same names tests/test_stratified_resources.py's test_the_default_kernels_keep_their_names looks for ...
    for flags in SHADE:
        for stats in (0, 1):
            _find(usage, f"10k_wf_shadeI{_args(stats, flags)}E")
            _find(usage, f"13k_wf_shade_stI{_args(stats, flags)}E")
    for flags in SHADOW:
        _find(usage, f"11k_wf_shadowI{_args(flags[0], flags[1:])}E")
        _find(usage, f"14k_wf_shadow_stI{_args(flags[0], flags[1:])}E")
    for frag in ("8k_wf_genILb0EE", "8k_wf_genILb1EE", "11k_wf_gen_stILb0EE", "11k_wf_gen_stILb1EE"):
        _find(usage, frag)
