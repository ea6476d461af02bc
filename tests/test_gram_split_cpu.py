"""csrc/gram_path.h, gram_share: which sub-chunks of a Gram task each wave of its workgroup walks when k_schur_gram splits the task (ba_kernels.h: SPLIT).
tests/native/gram_split_check.cpp, a stand-alone program under UBSan, checks for every task length 1..200 and 1..4 waves that the shares are disjoint and cover the
task, are whole sub-chunks except the task's last, and are empty exactly when there are more waves than sub-chunks."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shares_of_a_split_gram_task(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gram_split_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "gram_split_check.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and "GRAM_SPLIT_OK" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr


def test_split_kernels_fit_two_waves_per_simd_without_scratch():
    """k_schur_gram_split<...>: every instantiation within 256 registers, none with scratch but the three-tile class, which stays under the unsplit kernel's 40 B"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as KR
    lib = os.path.join(ROOT, "spherical_sfm_amd", "libssfm_hip.so")
    if not (os.path.exists(lib) and os.path.exists(KR.READELF)):
        pytest.skip("needs the built library and llvm-readelf")
    ks = {k["short"]: k for k in KR.kernels(lib).values() if k["short"].startswith("k_schur_gram_split")}
    expected = [f"k_schur_gram_split<{dc}, {nt}, {ti}, {fuse}>" for dc in (3, 6) for nt, ti in ((1, 0), (1, 2), (2, 0)) for fuse in (0, 1)]
    expected += ["k_schur_gram_split<6, 2, 3, 0>", "k_schur_gram_split<6, 2, 3, 1>", "k_schur_gram_split<6, 3, 0, 0>"]
    assert sorted(ks) == sorted(expected)
    for n, k in ks.items():
        assert k["vgpr"] + k["agpr"] <= 256 and not k["dynamic_stack"], (n, k)
        if n == "k_schur_gram_split<6, 3, 0, 0>":
            assert k["scratch"] <= 40, k
        else:
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k)
