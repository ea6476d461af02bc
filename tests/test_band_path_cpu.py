"""The plan of the reduced-system solve (csrc/band_path.h: factorisation kind, threads, LDS bytes, task sets of the back substitution, the substructured path and the
refactor rule) over both camera block sizes and half-widths 1..64, packed window on / off, substructured plan or not: the landmarks of the shipped decision and the
launch contracts the kernels state in their headers.  Host code, ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_path_landmarks_and_launch_contracts_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "band_path_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tests", "native", "band_path_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "BAND_PATH_OK" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr


def test_one_launch_site_per_band_kernel_family():
    """No launch macros in csrc/, and each of the reduced solve's kernel families is named in one function of reduced_solve.h only."""
    import re
    csrc = os.path.join(ROOT, "spherical_sfm_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".h", ".hip", ".cpp"))}
    assert not any(re.search(r"define SSFM_LAUNCH|define BACK_V2_LAUNCH", t) for t in text.values())
    src = text["reduced_solve.h"]
    # top-level functions of the file: a line that starts with `static` opens one, the next such line (or the end) closes it
    starts = [m.start() for m in re.finditer(r"^(?:template <[^\n]*>\n)?static ", src, re.M)] + [len(src)]
    for kernel in ("k_band_chol_v2<", "k_band_chol_v2p<", "k_band_back_v2<", "k_sub_sep_chain_mfma<", "k_sub_spike_fwd<"):
        owners = [i for i in range(len(starts) - 1) if kernel in src[starts[i]:starts[i + 1]]]
        assert len(owners) == 1, (kernel, owners)
        assert all(kernel not in t for f, t in text.items() if f != "reduced_solve.h" and f.endswith(".hip")), kernel
