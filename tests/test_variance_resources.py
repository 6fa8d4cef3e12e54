"""Build-time guard on the kernels of the measured variance (csrc/hrt_variance.hip), from hipcc's own resource report for
that unit alone (no GPU needed), read as tests/test_denoise_resources.py reads it: exactly the three streaming kernels, each without
scratch and without LDS, within the 64 VGPRs of eight waves per SIMD.  Prints the table DESIGN.md 4.13 quotes."""
import os
import re
import subprocess

import pytest

from tests.test_nee_resources import ROOT

SOURCE = os.path.join(ROOT, "hobbyraytracer_amd", "csrc", "hrt_variance.hip")
KERNELS = ("k_var_fold", "k_var_finish", "k_var_adaptive")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    out = tmp_path_factory.mktemp("variance_res") / "x.o"
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


def test_exactly_the_three_kernels_without_scratch_without_lds_within_64_vgprs(usage):
    src = open(SOURCE).read()
    assert src.count("__global__") == len(KERNELS) and src.count("__launch_bounds__(256)") == len(KERNELS)
    assert "__shared__" not in src and "atomic" not in src.replace("no atomics", "")
    assert len(usage) == len(KERNELS), sorted(usage)
    print(f"\n{'kernel':<16}{'VGPRs':>6}{'scratch':>8}{'LDS':>6}{'waves/SIMD':>11}")
    for k in KERNELS:
        hits = [(n, u) for n, u in usage.items() if k in n]
        assert len(hits) == 1, (k, sorted(usage))
        name, u = hits[0]
        print(f"{k:<16}{u['VGPRs']:>6}{u['ScratchSize']:>8}{u['LDS']:>6}{u['Occupancy']:>11}")
        assert u["ScratchSize"] == 0, (name, u)
        assert u["LDS"] == 0, (name, u)
        assert u["VGPRs"] <= 64, (name, u)
        assert u["Occupancy"] >= 8, (name, u)
