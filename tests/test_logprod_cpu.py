"""csrc/ssfm_math.h LogProd: the Cauchy cost of a lane's observations as ONE log of the product of its factors 1 + s/b (mantissa product + exponent sum) instead of one
log per observation.  tests/native/logprod_check.cpp, a stand-alone program under UBSan, holds the flushed total against the long-double sum of the logs of the same
factors: 1e4 factors in [1, 2), factors up to 1e300 (finite, no overflow), Cauchy-like mixes, all ones (exactly 0), inf and NaN (non-finite); relative error of the
total <= 1e-14 and the flush rules (every 1, 6, 64 factors) agreeing to the same bar."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_log_of_a_product_against_the_sum_of_logs(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "logprod_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "logprod_check.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and "LOGPROD_OK" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr
