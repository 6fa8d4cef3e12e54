"""Build-time guard on the id-matte kernel (k_aov_ids), from hipcc's own resource report of its translation unit (no
GPU needed), read as tests/test_nee_resources.py reads hrt_hip.hip's: both instantiations are there, keep the two 8-slot tables in
registers (no scratch), and fit the three blocks per CU their launch bound asks for, in registers and in LDS."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "hobbyraytracer_amd", "csrc", "hrt_aov_ids.hip")
WAVES = 3                                            # HRT_AOV_IDS_WAVES: __launch_bounds__(HRT_BLOCK, 3), k_aov's LDS-bounded residency
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    out = tmp_path_factory.mktemp("aov_ids_res") / "x.o"
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
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return res


def test_both_instantiations_have_no_scratch_and_fit_three_blocks_per_cu(usage):
    hits = {k: v for k, v in usage.items() if "k_aov_ids" in k}
    assert len(hits) == 2 and any("9k_aov_idsILb0E" in k for k in hits) and any("9k_aov_idsILb1E" in k for k in hits), list(usage)
    assert len(usage) == 2, list(usage)              # the unit holds nothing else
    src = open(SOURCE).read()
    assert re.search(r"#define HRT_AOV_IDS_WAVES %d\b" % WAVES, src) and "__launch_bounds__(HRT_BLOCK, HRT_AOV_IDS_WAVES)" in src
    for name, u in hits.items():
        print(f"{name}: {u}")
        assert u["ScratchSize"] == 0, (name, u)
        assert WAVES * u["LDS"] <= LDS_PER_CU, (name, u)
        assert u["VGPRs"] <= 512 // WAVES // 8 * 8, (name, u)      # 168: the registers of three waves per SIMD
        assert u["Occupancy"] >= WAVES, (name, u)
