"""Build-time guard on the kernels of environment-map sampling (HRT_FLAG_NEE_ENV), from hipcc's own resource report (no
GPU needed): its instantiations of k_wf_shade keep the shade budget (<= 128 VGPRs, no scratch), k_wf_shadow<true> with its second world_hit
and the CDF searches does not spill nor lose residency to its registers, and the table-build kernels use no scratch."""
import pytest

from tests.test_nee_resources import usage  # noqa: F401  (the module-scoped fixture: one hipcc run)


def _find(usage, frag):
    hits = {k: v for k, v in usage.items() if frag in k}
    assert hits, f"no {frag} in the report"
    return hits


@pytest.mark.parametrize("stats", [0, 1])
def test_env_shade_variant_keeps_the_shade_budget(usage, stats):
    # k_wf_shade<STATS, true, true>: 128 VGPRs, no scratch, with and without the counters
    for name, u in _find(usage, f"10k_wf_shadeILb{stats}ELb1ELb1E").items():
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 128, (name, u)


def test_env_shadow_kernel_keeps_its_residency(usage):
    # k_wf_shadow<true>: its LDS (stack, tables, queue) allows three blocks of four waves per CU; <= 168 VGPRs (512 / 3, in steps of 8)
    # keeps registers from lowering that (measured: 136 or 137 VGPRs, against 128 for k_wf_shadow<false>)
    for name, u in _find(usage, "11k_wf_shadowILb1E").items():
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 168, (name, u)
        assert 3 * u["LDS"] <= 160 * 1024, (name, u)


@pytest.mark.parametrize("frag", ["11k_wf_shadowILb0E", "10k_env_rows", "14k_env_marginal"])
def test_env_kernels_have_no_scratch(usage, frag):
    for name, u in _find(usage, frag).items():
        assert u["ScratchSize"] == 0, (name, u)
