"""Build-time guard on the kernels of the guided denoiser (csrc/hrt_denoise.hip), from hipcc's own resource report (no GPU
needed), read as tests/test_nee_resources.py reads it for hrt_hip.hip: every kernel keeps its state in registers (no scratch), within the
128 VGPRs of four waves per SIMD, and the LDS of the blocks per CU its launch bound asks for fits into the CU's 160 KB.  Prints the table
DESIGN.md 4.12 quotes."""
import os
import re
import subprocess

import pytest

from tests.test_nee_resources import ROOT

SOURCE = os.path.join(ROOT, "hobbyraytracer_amd", "csrc", "hrt_denoise.hip")
KERNELS = ("k_dn_prepare", "k_dn_variance", "k_dn_atrous", "k_dn_finish", "k_dn_resolve")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    out = tmp_path_factory.mktemp("denoise_res") / "x.o"
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
    return res


def test_every_kernel_is_in_the_report_without_scratch_within_128_vgprs_and_the_cus_lds(usage):
    src = open(SOURCE).read()
    waves = int(re.search(r"#define HRT_DN_WAVES (\d+)\b", src).group(1))          # blocks per CU the launch bound asks for (256 threads each)
    assert waves >= 4 and src.count("__launch_bounds__(256, HRT_DN_WAVES)") == 4
    assert len(usage) == len(KERNELS), sorted(usage)
    print(f"\n{'kernel':<16}{'VGPRs':>6}{'scratch':>8}{'LDS':>6}{'waves/SIMD':>11}")
    for k in KERNELS:
        hits = [(n, u) for n, u in usage.items() if k in n]
        assert len(hits) == 1, (k, sorted(usage))
        name, u = hits[0]
        print(f"{k:<16}{u['VGPRs']:>6}{u['ScratchSize']:>8}{u['LDS']:>6}{u['Occupancy']:>11}")
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs"] <= 128, (name, u)
        assert u["Occupancy"] >= 4, (name, u)
        blocks = waves if k != "k_dn_resolve" else 1
        assert blocks * u["LDS"] <= LDS_PER_CU, (name, u)
