"""Build-time guard on the kernels of the outlier filter (csrc/hrt_despeckle.hip), from hipcc's own resource report (no
GPU needed), read as tests/test_denoise_resources.py reads it: exactly the three kernels, each of which keeps its state -- the four
largest neighbours of k_ds_detect among it -- in registers (no scratch); the only LDS is k_ds_detect's 20 x 20 luminance tile; and the
VGPR and occupancy figures are the ones DESIGN.md 4.15 quotes.  Prints that table."""
import os
import re
import subprocess

import pytest

from tests.test_nee_resources import ROOT

SOURCE = os.path.join(ROOT, "hobbyraytracer_amd", "csrc", "hrt_despeckle.hip")
TILE_BYTES = 20 * 20 * 4
# kernel: (VGPRs, LDS bytes per block, waves per SIMD) -- the table of DESIGN.md 4.15
QUOTED = {"k_ds_luma": (7, 0, 8), "k_ds_detect": (22, TILE_BYTES, 8), "k_ds_apply": (27, 0, 8)}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    out = tmp_path_factory.mktemp("despeckle_res") / "x.o"
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


def test_exactly_three_kernels_without_scratch_with_one_lds_tile_and_the_quoted_registers(usage):
    src = open(SOURCE).read()
    assert src.count("__launch_bounds__(256, HRT_DS_WAVES)") == 3 and "asm" not in re.sub(r"//.*", "", src)
    assert len(usage) == len(QUOTED), sorted(usage)
    print(f"\n{'kernel':<14}{'VGPRs':>6}{'scratch':>8}{'LDS':>6}{'waves/SIMD':>11}")
    found = {}
    for k in QUOTED:
        hits = [(n, u) for n, u in usage.items() if k in n]
        assert len(hits) == 1, (k, sorted(usage))
        name, u = hits[0]
        print(f"{k:<14}{u['VGPRs']:>6}{u['ScratchSize']:>8}{u['LDS']:>6}{u['Occupancy']:>11}")
        assert u["ScratchSize"] == 0, (name, u)
        assert u["LDS"] <= (TILE_BYTES if k == "k_ds_detect" else 0), (name, u)
        found[k] = (u["VGPRs"], u["LDS"], u["Occupancy"])
    assert found == QUOTED
