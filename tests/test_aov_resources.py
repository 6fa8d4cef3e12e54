"""Build-time guard on the feature-buffer kernel (k_aov), from hipcc's own resource report (no GPU needed), read as
tests/test_roulette_resources.py reads it: both instantiations keep their state in registers (no scratch) and their LDS admits the
blocks per CU the launch bound asks for; and adding them moved no figure of any other kernel -- the report of every kernel whose name
does not contain k_aov equals the one compiled from the sources of the commit before."""
import os
import re
import subprocess

import pytest

from tests.test_nee_resources import ROOT, usage  # noqa: F401  (the module-scoped fixture: one hipcc run)

SOURCES = ("hobbyraytracer_amd/csrc", "include")     # everything hrt_hip.hip is compiled from
AOV_WAVES = 3                                        # HRT_AOV_WAVES: k_aov's __launch_bounds__(HRT_BLOCK, 3) = three blocks of four waves per CU
LDS_PER_CU = 160 * 1024


def _aov(usage):  # noqa: F811
    hits = {k: v for k, v in usage.items() if "k_aov" in k}
    assert len(hits) == 2 and any("5k_aovILb0E" in k for k in hits) and any("5k_aovILb1E" in k for k in hits), list(hits)
    return hits


def test_both_instantiations_have_no_scratch_and_the_lds_of_three_blocks_per_cu(usage):  # noqa: F811
    src = open(os.path.join(ROOT, "hobbyraytracer_amd", "csrc", "hrt_hip.hip")).read()
    assert re.search(r"#define HRT_AOV_WAVES %d\b" % AOV_WAVES, src) and "__launch_bounds__(HRT_BLOCK, HRT_AOV_WAVES)" in src
    for name, u in _aov(usage).items():
        print(f"{name}: {u}")
        assert u["ScratchSize"] == 0, (name, u)
        assert AOV_WAVES * u["LDS"] <= LDS_PER_CU, (name, u)
        assert u["VGPRs"] <= 512 // AOV_WAVES // 8 * 8, (name, u)      # 168: the registers of three waves per SIMD


def _git(*args):
    return subprocess.run(["git", "-C", ROOT, *args], capture_output=True)


def _parent_sources(dest):
    """The sources of the newest of HEAD, HEAD~ that differ from the working tree's, unpacked under dest -> the revision's name.  Skips,
    with the reason, when git cannot tell or when both revisions hold the working tree's sources (there is then no parent to compare)."""
    ls = _git("ls-files", "--cached", "--others", "--exclude-standard", "--", *SOURCES)      # every directory level, no build products
    if ls.returncode != 0:
        pytest.skip(f"the parent commit is not reachable: git ls-files: {ls.stderr.decode().strip()[-200:]}")
    here = {}
    for n in ls.stdout.decode().splitlines():
        if os.path.isfile(os.path.join(ROOT, n)):
            with open(os.path.join(ROOT, n), "rb") as f:
                here[n] = f.read()
    for rev in ("HEAD", "HEAD~"):
        ls = _git("ls-tree", "-r", "--name-only", rev, "--", *SOURCES)
        if ls.returncode != 0:
            pytest.skip(f"the parent commit is not reachable: git ls-tree {rev}: {ls.stderr.decode().strip()[-200:]}")
        blobs = {}
        for n in ls.stdout.decode().splitlines():
            show = _git("show", f"{rev}:{n}")
            if show.returncode != 0:
                pytest.skip(f"the parent commit is not reachable: git show {rev}:{n}")
            blobs[n] = show.stdout
        if blobs != here:
            for n, b in blobs.items():
                path = os.path.join(dest, n)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with open(path, "wb") as f:
                    f.write(b)
            return rev
    pytest.skip("HEAD and HEAD~ both hold the working tree's sources: there is no parent to compare the report with")


def test_no_other_kernel_moved(usage, tmp_path):  # noqa: F811
    rev = _parent_sources(str(tmp_path))
    hip = os.path.join(str(tmp_path), "hobbyraytracer_amd", "csrc", "hrt_hip.hip")
    # (device code only: the report is the device compiler's)
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-ffp-contract=off",
           "-Wno-unused-value", "-I" + os.path.join(str(tmp_path), "include"), "-c", hip, "-o", os.path.join(str(tmp_path), "parent.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    parent, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); parent[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            parent[name][m.group(1).split(" ")[0]] = int(m.group(2))
    assert parent, "hipcc printed no resource report for " + rev
    mine = {k: v for k, v in usage.items() if "k_aov" not in k}
    parent = {k: v for k, v in parent.items() if "k_aov" not in k}
    assert sorted(mine) == sorted(parent), (sorted(set(mine) ^ set(parent)), rev)
    moved = {k: (parent[k], mine[k]) for k in mine if mine[k] != parent[k]}
    assert not moved, (moved, rev)
