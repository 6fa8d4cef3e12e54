"""Build-time guard on the kernels of next-event estimation (HRT_FLAG_NEE), from hipcc's own resource report (no
GPU needed): the NEE instantiation of k_wf_shade keeps the default's budget (<= 128 VGPRs: 4 waves per SIMD, no scratch), and
k_wf_shadow, which traces one world_hit per eligible vertex, does not spill."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    out = tmp_path_factory.mktemp("nee_res") / "x.o"
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value",
           "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "hobbyraytracer_amd", "csrc", "hrt_hip.hip"), "-o", str(out),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return res


def test_nee_shade_variant_keeps_the_shade_budget(usage):
    hits = {k: v for k, v in usage.items() if "10k_wf_shadeILb0ELb1E" in k}
    assert hits, "no k_wf_shade<false, true> (the NEE instantiation) in the report"
    for name, u in hits.items():
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 128, (name, u)


def test_shadow_kernel_has_no_scratch(usage):
    hits = {k: v for k, v in usage.items() if "11k_wf_shadow" in k}
    assert hits, "no k_wf_shadow in the report"
    for name, u in hits.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert 3 * u["LDS"] <= 160 * 1024, (name, u)     # three blocks per CU
