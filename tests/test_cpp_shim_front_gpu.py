"""The C++ mirror of the pairwise front end on the GPU.  run_spherical_sfm -match: the driver starts from keyframes.txt + features.dat alone (match_exhaustive + estimate_pairwise in one device call, then
find_largest_connected_component) and must arrive where the same driver arrives from a matches.dat that holds the same exhaustive matches (-pairwise).
demo_match drives the mirrors of match / match_exhaustive on keyframes whose frame
numbers are not their positions, against tests/_match_ref.py, and feeds the result through estimate_pairwise."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _front_scene as S
import _match_ref as MR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(outdir, frames, matches=None, indices=None, shift=(0.0, 0.0)):
    os.makedirs(outdir, exist_ok=True)
    indices = list(range(len(frames))) if indices is None else indices
    with open(os.path.join(outdir, "keyframes.txt"), "w") as f:
        f.write("%d\n" % len(frames))
        for i in indices:
            f.write("%d %06d.jpg\n" % (i, i + 1))
    with open(os.path.join(outdir, "features.dat"), "wb") as f:
        for xy, d in frames:
            f.write(struct.pack("i", len(xy)))
            for k in range(len(xy)):
                f.write(np.asarray(xy[k] + np.asarray(shift), np.float32).tobytes()); f.write(np.asarray(d[k], np.float32).tobytes())
    if matches is not None:
        with open(os.path.join(outdir, "matches.dat"), "wb") as f:
            f.write(struct.pack("i", len(matches)))
            for (a, b, j, i) in matches:
                f.write(struct.pack("3i", a, b, len(j)))
                f.write(np.stack([j, i], axis=1).astype(np.int32).tobytes())
                f.write(np.eye(3).tobytes())
    with open(os.path.join(outdir, "intrinsics.txt"), "w") as f:
        f.write("%.17g %.17g %.17g\n" % (S.FOCAL, S.CX, S.CY))


def _exe(name):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    exe = os.path.join(ROOT, "spherical_sfm_amd", name)
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    return exe


def _result(stdout, tag):
    lines = [l for l in stdout.splitlines() if l.startswith(tag)]
    assert len(lines) == 1, stdout[-2000:]
    return lines[0], dict(x.split("=") for x in lines[0].split()[1:])


def _run(exe, out, flag):
    # Two processes are compared bit for bit, down to poses.txt after four bundle adjustments.  The BA's default assembly adds with fp64 atomics and is
    # reproducible only to a few ulp from run to run ("Tolerances a caller can rely on"); SSFM_DETERMINISTIC=1 is the library's mode for
    # bit-identical repeats.  Everything before the BA (matching, LO-MSAC, component, rotation averaging) is bit-reproducible in either mode.
    res = subprocess.run([exe, "-intrinsics", os.path.join(out, "intrinsics.txt"), "-output", out, "-inlierthresh", "2", "-mininliers", "20", flag],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, SSFM_DETERMINISTIC="1"))
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return _result(res.stdout, "PAIRWISE_RESULT")[0], open(os.path.join(out, "poses.txt")).read()


def test_match_flag_equals_the_run_from_the_same_matches(tmp_path):
    exe = _exe("run_spherical_sfm")
    N = 12
    frames = S.ring_frames(N, per_cam=60, stray=True)                         # 12 ring frames + 2 frames that only match each other
    # the pixel positions go through float32 in features.dat: the matcher and both runs see the same values
    a = str(tmp_path / "from_features"); _write(a, frames)
    pw_a, poses_a = _run(exe, a, "-match")
    # The same exhaustive matches, by the numpy matcher.  The -pairwise path has no component step, so it is given what the largest component keeps: the ring
    # frames alone (a pair's matches do not depend on which other frames exist).
    pairs = MR.exhaustive_pairs(N)
    mp, m0, m1 = MR.match_pairs([f[1] for f in frames[:N]], pairs)
    matches = [(p[0], p[1], m0[mp[k]:mp[k + 1]], m1[mp[k]:mp[k + 1]]) for k, p in enumerate(pairs) if mp[k + 1] > mp[k]]
    b = str(tmp_path / "from_matches"); _write(b, frames[:N], matches)
    pw_b, poses_b = _run(exe, b, "-pairwise")
    assert pw_a == pw_b, (pw_a, pw_b)
    assert poses_a == poses_b
    kv = dict(x.split("=") for x in pw_a.split()[1:])
    assert int(kv["pairs"]) >= N and int(kv["loop_closures"]) >= 1            # (i, i+1) around the ring, (i, i+2) and the wrap-around as closures
    poses = np.loadtxt(os.path.join(a, "poses.txt"))
    assert poses.shape[0] == N and np.array_equal(poses[:, 0].astype(int), np.arange(N))      # the stray frames 12, 13 are gone


def test_match_mirrors_with_frame_numbers_that_are_not_positions(tmp_path):
    """match / match_exhaustive of shim/tools.h: keyframes.txt carries the frame numbers 3, 7, 8, 20, 21, 40; the ImageMatch indices must be POSITIONS (what
    estimate_pairwise and everything after it index `keyframes` with).  Lists against the numpy matcher, every pair stored (also the empty ones); then
    match_exhaustive + estimate_pairwise against estimate_pairwise_from_features: the same ImageMatches, rotations bit for bit."""
    exe = _exe("demo_match")
    frames = S.arc_frames((130, 70, 130, 2, 0, 70), dim=128, seed=5)
    out = str(tmp_path / "m"); _write(out, frames, indices=[3, 7, 8, 20, 21, 40])
    res = subprocess.run([exe, out, "%.17g" % S.FOCAL, "%.17g" % S.CX, "%.17g" % S.CY, "2", "10"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    r = _result(res.stdout, "DEMO_MATCH_RESULT")[1]
    pairs = MR.exhaustive_pairs(len(frames))
    mp, m0, m1 = MR.match_pairs([f[1] for f in frames], pairs)
    want = ["%d %d %d" % (a, b, mp[k + 1] - mp[k]) + "".join(" %d %d" % (j, i) for j, i in zip(m0[mp[k]:mp[k + 1]], m1[mp[k]:mp[k + 1]])) for k, (a, b) in enumerate(pairs)]
    got = open(os.path.join(out, "match_exhaustive.txt")).read().splitlines()
    assert got == want
    assert any(l.split()[2] == "0" for l in got) and int(r["pairs"]) == len(pairs) == 15
    j, i = MR.match_pair(frames[0][1], frames[1][1], 1.5)
    assert open(os.path.join(out, "match_ratio.txt")).read().split() == [str(x) for x in [0, 1, len(j)] + [v for ji in zip(j, i) for v in ji]]
    assert r["match_same"] == "1" and r["equal"] == "1" and r["accepted_a"] == r["accepted_b"] and int(r["accepted_a"]) >= 3
