"""Build-time guard on k_wf_merge (csrc/hrt_merge.hip), from hipcc's own resource report for that unit alone (no GPU
needed), read as tests/test_variance_resources.py reads it: exactly the one kernel, a plain streaming copy -- no scratch, no LDS, within
the 64 VGPRs of eight waves per SIMD."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_resources import ROOT

SOURCE = os.path.join(ROOT, "hobbyraytracer_amd", "csrc", "hrt_merge.hip")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    out = tmp_path_factory.mktemp("merge_res") / "x.o"
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-ffp-contract=off",
           "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"), "-c", SOURCE, "-o", str(out), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" ")[0]] = int(m.group(2))
    assert res, "hipcc printed no resource report"
    return res


def test_merge_kernel_has_no_scratch_no_lds_and_at_most_64_vgprs(usage):
    src = open(SOURCE).read()
    assert src.count("__global__") == 1 and "__shared__" not in src and "atomic" not in src
    assert len(usage) == 1, sorted(usage)
    for name, u in usage.items():
        print(f"\n{name}: {u}")
        assert "k_wf_merge" in name
        assert u["ScratchSize"] == 0, (name, u)
        assert u["LDS"] == 0, (name, u)
        assert u["VGPRs"] <= 64, (name, u)
