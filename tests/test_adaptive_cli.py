"""CLI flags of adaptive sampling that are refused before any device is touched (exit 2), and what runs without a GPU:
the scene loads, the adaptive ABI is declared and its struct has the header's layout."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags, message", [
    (["--adaptive", "0.1", "--gpus", "2"], "--gpus"),
    (["--adaptive", "0.1", "--checkpoint", "ck.bin"], "--checkpoint"),
    (["--adaptive", "0.1", "--checkpoint", "ck.bin", "--resume"], "--checkpoint"),
    (["--adaptive", "0.1", "--resume"], "--resume"),
    (["--adaptive", "abc"], "--adaptive"),
    (["--adaptive", "-0.5"], "--adaptive"),
    (["--adaptive", "nan"], "--adaptive"),
    (["--adaptive", "0.1x"], "--adaptive"),
    (["--adaptive", "0.1", "--min-samples", "1"], "--min-samples"),
    (["--sample-map", "m.pfm"], "--sample-map"),
])
def test_refused_combinations(built, scenes_dir, tmp_path, flags, message):
    from hobbyraytracer_amd import api
    r = subprocess.run([api.CLI_PATH, os.path.join(scenes_dir, "cornell_box.yaml"), "--size", "16x16"] + flags, cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stdout + r.stderr
    err = r.stderr.strip().splitlines()
    assert len(err) == 1 and message in err[0], r.stderr
    assert "Loaded scene" not in r.stdout            # refused before the scene (and any device) is touched
    assert not os.listdir(tmp_path)


def test_adaptive_needs_two_samples(built, scenes_dir, tmp_path):
    """--adaptive with 1 spp is refused after the scene loaded (that is where the spp is known), before the render."""
    from hobbyraytracer_amd import api
    r = subprocess.run([api.CLI_PATH, os.path.join(scenes_dir, "cornell_box.yaml"), "--size", "16x16", "--spp", "1", "--adaptive", "0.1"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "at least 2 samples" in r.stderr, r.stdout + r.stderr
    assert "Loaded scene" in r.stdout


def test_adaptive_struct_layout(built, tmp_path):
    """hrt_adaptive of include/hrt.h and api.Adaptive agree (size and offsets), and the library exports the three entry points."""
    import ctypes as C
    from hobbyraytracer_amd import api
    src = tmp_path / "a.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/hrt.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(hrt_adaptive), offsetof(hrt_adaptive, min_samples),'
                   ' offsetof(hrt_adaptive, pass_samples), offsetof(hrt_adaptive, threshold), offsetof(hrt_adaptive, floor)); return 0;}\n')
    exe = tmp_path / "a"
    subprocess.check_call(["cc", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(api.Adaptive)] + [getattr(api.Adaptive, f).offset for f in ("min_samples", "pass_samples", "threshold", "floor")]
    lib = C.CDLL(api.HIP_LIB_PATH)
    for name in ("hrt_render_stripes_adaptive_device", "hrt_render_stripes_adaptive", "hrt_adaptive_mean_device"):
        assert hasattr(lib, name)


def test_adaptive_kernels_do_not_spill(tmp_path):
    """The new kernels compile for gfx950 without scratch (hipcc's resource report, as tests/test_kernel_resources.py reads it)."""
    import re
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value",
           "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "hobbyraytracer_amd", "csrc", "hrt_hip.hip"), "-o", str(tmp_path / "x.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize)[^:]*: (\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    for frag in ("k_wf_reduce_list", "k_ad_selectILi0", "k_ad_selectILi1", "k_ad_scan", "k_ad_mean"):
        hits = {k: v for k, v in res.items() if frag in k}
        assert hits, frag
        for k, v in hits.items():
            assert v["ScratchSize"] == 0 and v["VGPRs"] <= 64, (k, v)
