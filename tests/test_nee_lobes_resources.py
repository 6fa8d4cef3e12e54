"""Build-time guard on the kernels of HRT_FLAG_NEE_LOBES, from hipcc's own resource report (no GPU needed), read as
tests/test_nee_resources.py reads it: every k_wf_shade<false, true, ENV, EMIT, true> keeps the shade budget (<= 128 VGPRs: 4 waves per
SIMD; no scratch), its counters variant takes no more scratch than the same kernel without LOBES (the 20 B stack object of the
HRT_FLAG_NEE counters kernel, not a register spill), and every k_wf_shadow<ENV, EMIT, true> keeps three blocks per CU (<= 168 VGPRs,
no scratch, LDS).  The figures are printed: DESIGN.md 4.8 quotes them."""
import pytest

from tests.test_nee_resources import usage  # noqa: F401  (the module-scoped fixture: one hipcc run)


def _find(usage, frag):
    hits = {k: v for k, v in usage.items() if frag in k}
    assert hits, f"no {frag} in the report"
    return hits


@pytest.mark.parametrize("env", [0, 1])
@pytest.mark.parametrize("emit", [0, 1])
def test_lobes_shade_variants_keep_the_shade_budget(usage, env, emit):
    for name, u in _find(usage, f"10k_wf_shadeILb0ELb1ELb{env}ELb{emit}ELb1EE").items():
        print(f"k_wf_shade<false, true, {env}, {emit}, true>: {u}")
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 128, (name, u)
    plain = max(u["ScratchSize"] for u in _find(usage, f"10k_wf_shadeILb1ELb1ELb{env}ELb{emit}ELb0EE").values())
    for name, u in _find(usage, f"10k_wf_shadeILb1ELb1ELb{env}ELb{emit}ELb1EE").items():
        print(f"k_wf_shade<true, true, {env}, {emit}, true>: {u}")
        assert u["VGPRs"] <= 128 and u["ScratchSize"] <= plain, (name, u, plain)


@pytest.mark.parametrize("env", [0, 1])
@pytest.mark.parametrize("emit", [0, 1])
def test_lobes_shadow_kernels_keep_their_residency(usage, env, emit):
    for name, u in _find(usage, f"11k_wf_shadowILb{env}ELb{emit}ELb1EE").items():
        print(f"k_wf_shadow<{env}, {emit}, true>: {u}")
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 168, (name, u)
        assert 3 * u["LDS"] <= 160 * 1024, (name, u)


def test_kernels_without_the_flag_are_still_instantiated(usage):
    # the LOBES parameter is a trailing default: the kernels the other flags launch keep their own instantiations
    for frag in ("10k_wf_shadeILb0ELb0ELb0ELb0ELb0EE", "10k_wf_shadeILb0ELb1ELb0ELb0ELb0EE", "11k_wf_shadowILb0ELb0ELb0EE", "11k_wf_shadowILb1ELb1ELb0EE"):
        _find(usage, frag)
