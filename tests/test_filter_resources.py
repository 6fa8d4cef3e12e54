"""Build-time guard on the kernels of the reconstruction filter (csrc/hrt_filter.hip), from hipcc's own resource report
(no GPU needed), read as tests/test_despeckle_resources.py reads it: the gather and the finishing kernel, each in its three window
sizes and two samplers; none of them spills (no scratch); the LDS of a block is its staged halo and nothing else -- per cell the
jitter (8 bytes), the 1-D weights of its 2 (2N + 1) offsets (4 bytes each) and, in the gather, the sample's value (16) -- which admits
at least six blocks on a CU's 160 KB where DESIGN.md 4.16 asks for at least four; and both state __launch_bounds__(256) and hold no
atomics.  Prints the table."""
import os
import re
import subprocess

import pytest

from tests.test_nee_resources import ROOT

SOURCE = os.path.join(ROOT, "hobbyraytracer_amd", "csrc", "hrt_filter.hip")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    out = tmp_path_factory.mktemp("filter_res") / "x.o"
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


def test_twelve_kernels_without_scratch_whose_lds_is_the_staged_halo(usage):
    src = re.sub(r"//.*", "", open(SOURCE).read())
    assert src.count("__global__ __launch_bounds__(256)") == 2 and "asm" not in src and "atomic" not in src
    assert len(usage) == 12, sorted(usage)
    print(f"\n{'kernel':<16}{'N':>2}{'strat':>6}{'VGPRs':>6}{'scratch':>8}{'LDS':>6}{'blocks/CU by LDS':>17}{'waves/SIMD':>11}")
    for kernel, fixed in (("k_flt_gather", 24), ("k_flt_finish", 8)):
        for n in (0, 1, 2):
            for strat in (0, 1):
                hits = [(name, u) for name, u in usage.items() if f"{kernel}ILi{n}ELb{strat}E" in name]
                assert len(hits) == 1, (kernel, n, strat, sorted(usage))
                name, u = hits[0]
                blocks = LDS_PER_CU // u["LDS"]
                print(f"{kernel:<16}{n:>2}{strat:>6}{u['VGPRs']:>6}{u['ScratchSize']:>8}{u['LDS']:>6}{blocks:>17}{u['Occupancy']:>11}")
                assert u["ScratchSize"] == 0, (name, u)
                assert u["LDS"] == (fixed + 8 * (2 * n + 1)) * (16 + 2 * n) ** 2, (name, u)
                assert blocks >= 4, (name, u)
                assert u["Occupancy"] >= 4, (name, u)          # registers admit the four blocks (of four waves) per CU too
