"""The C++ mirror of the five-point front end on the GPU: estimate_pairwise_five_point_from_features (shim/tools.h) through the third part of demo_match, on the
scene and arguments of tests/test_fivepoint_shim_gpu.py (on the CPU: 5 candidates with 22, 42, 16, 23 and 19 matches, none marginal, all accepted), against
the two-call mirror match_exhaustive + estimate_pairwise_five_point that the same run computes.  (run_spherical_sfm_uncalib -match -fivepoint, which now goes
through the new mirror, is held by test_uncalibrated_driver_with_match_and_fivepoint_runs_to_poses there.)"""
import os
import struct
import subprocess

import numpy as np
import pytest

import _front_scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(outdir, frames, indices):
    """keyframes.txt + features.dat as tests/test_fivepoint_shim_gpu.py writes them"""
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "keyframes.txt"), "w") as f:
        f.write("%d\n" % len(frames))
        for i in indices:
            f.write("%d %06d.jpg\n" % (i, i + 1))
    with open(os.path.join(outdir, "features.dat"), "wb") as f:
        for xy, d in frames:
            f.write(struct.pack("i", len(xy)))
            for k in range(len(xy)):
                f.write(np.asarray(xy[k], np.float32).tobytes()); f.write(np.asarray(d[k], np.float32).tobytes())


def _exe(name):
    exe = os.path.join(ROOT, "spherical_sfm_amd", name)
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    return exe


def test_demo_match_front_part_equals_the_two_call_mirror(gpu_ctx, tmp_path):
    MIN = 10
    frames = S.arc_frames((130, 70, 130, 2, 0, 70), dim=128, seed=5)
    out = str(tmp_path / "m"); _write(out, frames, indices=[3, 7, 8, 20, 21, 40])
    res = subprocess.run([_exe("demo_match"), out, "%.17g" % S.FOCAL, "%.17g" % S.CX, "%.17g" % S.CY, "2", str(MIN)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("DEMO_FIVEPOINT_FRONT_RESULT")]
    assert len(line) == 1, res.stdout[-2000:]
    kv = dict(x.split("=") for x in line[0].split()[1:])
    assert kv["equal"] == "1" and int(kv["accepted"]) >= 3, line[0]
    front = open(os.path.join(out, "five_point_front.txt"), "rb").read(); two = open(os.path.join(out, "five_point.txt"), "rb").read()
    assert front == two and len(front.splitlines()) == int(kv["accepted"])
    # the older parts of the demo still print their own lines, one each
    assert sum(l.startswith("DEMO_MATCH_RESULT") for l in res.stdout.splitlines()) == 1 and sum(l.startswith("DEMO_FIVEPOINT_RESULT") for l in res.stdout.splitlines()) == 1
