"""The plan of the signature-group assembly and its back substitution (csrc/gram_path.h: tile classes, the LDS slice of a wave, the Gram launches with their waves per
task, grids and bytes, the grouped back substitution) against a second implementation of its rules, over both camera block sizes, task sets of one / all / some
classes, task counts on both sides of every threshold and every knob; the landmarks of the shipped decision, the launch contracts, the cost model's class and the
slice layout with the overlay of G.  Host code, ASan + UBSan; a row stride too small for the overlay must not compile."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "gram_path_check.cpp")
FLAGS = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_gram_path_against_second_implementation_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gram_path_check")
    cc = subprocess.run(FLAGS + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "GRAM_PATH_OK" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr


def test_row_stride_too_small_for_the_overlay_does_not_compile(tmp_path):
    """SSFM_GRAM_LD=24: G of a K = 8 task would run over the scales and the slot tables of its slice -- a static_assert, not a silent overrun"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    cc = subprocess.run(FLAGS + ["-DSSFM_GRAM_LD=24", "-fsyntax-only", SRC], capture_output=True, text=True, timeout=300)
    assert cc.returncode != 0 and "SSFM_GRAM_LD is too small" in cc.stderr, cc.stderr[-3000:]


def test_tile_class_rule_written_once():
    """Outside gram_path.h nothing in csrc/ compares the rows of a Gram task with a class bound, except the cascade k_schur_gram_any keeps for its register allocation."""
    import re
    csrc = os.path.join(ROOT, "spherical_sfm_amd", "csrc")
    hits = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".h", ".hip", ".cpp")) or f == "gram_path.h":
            continue
        for n, line in enumerate(open(os.path.join(csrc, f)), 1):
            if re.search(r"\brows\s*<=?\s*(16|20|32|36)\b", line):
                hits.append((f, n))
    lines = open(os.path.join(csrc, "ba_kernels.h")).read().splitlines()
    lo = next(i for i, l in enumerate(lines, 1) if l.startswith("#define SSFM_GRAM_ANY"))
    hi = next(i for i, l in enumerate(lines, 1) if l.startswith("#undef SSFM_GRAM_ANY"))
    assert len(hits) == 4 and all(f == "ba_kernels.h" and lo < n < hi for f, n in hits), hits
