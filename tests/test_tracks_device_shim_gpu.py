"""run_spherical_sfm with and without -devicetracks on the same feature-track directory: build_sfm's track pass on the device (ssfm_build_tracks_device through
the C++ mirror) feeds Retriangulate and Optimize the same problem as the host pass, up to the numbering and order of the points."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(exe, out, *flags):
    res = subprocess.run([exe, "-intrinsics", os.path.join(out, "intrinsics.txt"), "-output", out, *flags], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("PIPELINE_RESULT")][0]
    return dict(kv.split("=") for kv in line.split()[1:]), res.stdout


def test_driver_with_device_tracks_matches_the_host_pass(tmp_path):
    from _tracks_dataset import write_tracks
    exe = os.path.join(ROOT, "spherical_sfm_amd", "run_spherical_sfm")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    host_dir = str(tmp_path / "host"); dev_dir = str(tmp_path / "device")
    # no wrong matches.  Tracks of 5 cameras: at 40 cameras (9 degrees apart) the generator's default of 6 leaves the 1920 x 1080 frame and is refused
    write_tracks(host_dir, 40, 1500, K=5)
    shutil.copytree(host_dir, dev_dir)
    h, h_out = run(exe, host_dir)
    d, d_out = run(exe, dev_dir, "-devicetracks")
    assert "device tracks:" in d_out and "device tracks:" not in h_out
    assert h["ok"] == d["ok"] == "1111" and h["cameras"] == d["cameras"] == "40" and h["residuals"] == d["residuals"]
    # the same set of residuals in another point order: the two solves can stop one iteration apart and no further -- the solver's own function_tolerance
    for k in ("cost_spherical", "cost_general"):
        a, b = float(h[k]), float(d[k])
        assert abs(a - b) <= 1e-6 * max(abs(a), abs(b)), (k, a, b)
    # (the point counts are not compared: the host path counts issued ids)
