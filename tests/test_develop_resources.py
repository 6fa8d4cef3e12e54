"""Build-time guard on the kernels of the develop stage (csrc/hrt_develop.hip), from hipcc's own resource report (no GPU
needed), read as tests/test_despeckle_resources.py reads it: exactly the six kernels DESIGN lists, none with scratch; LDS only where
DESIGN says -- the block's 2048-bin histogram of k_dv_meter_film and the scan and partial sums of the one-block k_dv_meter --; and the
VGPR and occupancy figures are the ones DESIGN.md 4.17 quotes.  Prints that table."""
import os
import re
import subprocess

import pytest

from tests.test_nee_resources import ROOT

SOURCE = os.path.join(ROOT, "hobbyraytracer_amd", "csrc", "hrt_develop.hip")
HIST_BYTES = 2048 * 4
METER_BYTES = 256 * 4 + 2 * 256 * 8
# kernel: (VGPRs, LDS bytes per block, waves per SIMD) -- the table of DESIGN.md 4.17
QUOTED = {"k_dv_down_film": (35, 0, 8), "k_dv_down": (68, 0, 7), "k_dv_up_add": (22, 0, 8), "k_dv_meter_film": (28, HIST_BYTES, 8),
          "k_dv_meter": (62, METER_BYTES, 8), "k_dv_write": (26, 0, 8)}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    out = tmp_path_factory.mktemp("develop_res") / "x.o"
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


def test_exactly_the_six_kernels_without_scratch_with_lds_only_in_the_meter_and_the_quoted_registers(usage):
    src = re.sub(r"//.*", "", open(SOURCE).read())
    assert src.count("__launch_bounds__(HRT_DV_BLOCK, HRT_DV_WAVES)") == len(QUOTED) == src.count("__global__") and "asm" not in src
    assert "atomicAdd" in src and not re.search(r"atomic\w*\(\s*\(?\s*float|unsafeAtomic|atomicAdd_f", src)     # integer atomics only
    assert len(usage) == len(QUOTED), sorted(usage)
    print(f"\n{'kernel':<17}{'VGPRs':>6}{'scratch':>8}{'LDS':>6}{'waves/SIMD':>11}")
    found = {}
    for k in QUOTED:
        hits = [(n, u) for n, u in usage.items() if re.search(r"\d" + k + "E", n)]
        assert len(hits) == 1, (k, sorted(usage))
        name, u = hits[0]
        print(f"{k:<17}{u['VGPRs']:>6}{u['ScratchSize']:>8}{u['LDS']:>6}{u['Occupancy']:>11}")
        assert u["ScratchSize"] == 0, (name, u)
        assert u["LDS"] <= QUOTED[k][1], (name, u)
        found[k] = (u["VGPRs"], u["LDS"], u["Occupancy"])
    assert found == QUOTED
