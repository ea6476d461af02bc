"""bench.py as the driver runs it: a plain run times exactly --steps steps, prints the headline record and, with --dump-outputs, writes what
the last timed step computed (float64 .npy files) -- here checked against the oracle's solve of the same seeded problem."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path, oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    # a small circle keeps the run short; the code path is the headline's
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--cameras", "60", "--points", "4000",
           "--dump-outputs", str(tmp_path / "out")]
    detail = os.path.join(ROOT, "bench_detail.json")
    before = os.path.getmtime(detail) if os.path.exists(detail) else None
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["unit"] == "obs/s"
    assert "roofline" not in rec and "cpu_baseline" not in rec and "detail" not in rec
    assert (os.path.getmtime(detail) if os.path.exists(detail) else None) == before                 # the detail file is --full's
    assert sorted(os.listdir(tmp_path / "out")) == ["cameras.npy", "focal.npy", "points.npy", "summary.npy"]
    out = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in ("cameras", "points", "focal", "summary")}
    assert all(a.dtype == np.float64 for a in out.values())
    from spherical_sfm_amd import synth
    p = synth.make_circle(60, 4000, 6, spherical=False, focal_fixed=True)
    oc, op, of, os_ = oracle.ba_solve(p)
    assert out["cameras"].shape == oc.shape and out["points"].shape == op.shape and out["focal"][0] == pytest.approx(of, rel=1e-12)
    assert np.abs(out["cameras"] - oc).max() / np.abs(oc).max() <= 1e-5
    assert (np.linalg.norm(out["points"] - op, axis=1) / np.linalg.norm(op, axis=1)).max() <= 1e-5
    assert out["summary"][2] == os_["iterations"] and out["summary"][1] < out["summary"][0]
