"""Build-time guard on the kernels of the emitter table (HRT_FLAG_NEE_EMITTERS), from hipcc's own resource report (no GPU
needed): its instantiations of k_wf_shade keep the shade budget (<= 128 VGPRs: 4 waves per SIMD; no scratch, except the
counters variant without ENV, which keeps the existing NEE counters kernel's 20 B stack object), and k_wf_shadow<ENV, true> keeps three blocks per CU (<= 168 VGPRs, no scratch)."""
import pytest

from tests.test_nee_resources import usage  # noqa: F401  (the module-scoped fixture: one hipcc run)


def _find(usage, frag):
    hits = {k: v for k, v in usage.items() if frag in k}
    assert hits, f"no {frag} in the report"
    return hits


@pytest.mark.parametrize("env", [0, 1])
def test_emitter_shade_variant_keeps_the_shade_budget(usage, env):
    for name, u in _find(usage, f"10k_wf_shadeILb0ELb1ELb{env}ELb1E").items():
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 128, (name, u)
    # with the counters: no scratch with ENV; without ENV the 20 B stack object of the HRT_FLAG_NEE counters kernel k_wf_shade<true, true>
    # (below 128 VGPRs: not a register spill), and never more than it
    nee_stats = max(u["ScratchSize"] for u in _find(usage, f"10k_wf_shadeILb1ELb1ELb{env}ELb0E").values())
    for name, u in _find(usage, f"10k_wf_shadeILb1ELb1ELb{env}ELb1E").items():
        assert u["VGPRs"] <= 128 and u["ScratchSize"] <= nee_stats and (env == 0 or u["ScratchSize"] == 0), (name, u, nee_stats)


@pytest.mark.parametrize("env", [0, 1])
def test_emitter_shadow_kernel_keeps_its_residency(usage, env):
    for name, u in _find(usage, f"11k_wf_shadowILb{env}ELb1E").items():
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 168, (name, u)
        assert 3 * u["LDS"] <= 160 * 1024, (name, u)
