"""run_spherical_sfm_uncalib -viewgraph -rotinit l1 (find_best_focal_length_random_l1 -> ssfm_focal_search_l1) on feature tracks whose matches carry wrong rotations.
The scene is the one of tests/test_view_graph_gpu.py::test_uncalibrated_driver_with_viewgraph_recovers_the_focal (tests/_tracks_dataset.py: matches estimated at the
guessed focal 1500, true focal 1000, cameras renumbered, match list shuffled) with the neighbours at distance 1-5 matched (300 matches), 30 of which are rotated
by a further 20-170 degrees.

The numpy restatement (tests/_focal_l1_ref.py) on these matches, over the driver's range 375-3000: the tree search's cost is smallest at 375; the L1 cost is a V with
its tip at 1000 (41.09; 41.49 at 990, 41.62 at 1010, 59.7 at 375), about 0.05 per pixel of focal, so the best of 1024 uniform trials (2.6 pixels apart on average)
lies within 10 pixels of 1000.  At the true focal the converged residuals of the clean matches stay below 2 degrees and those of the corrupted ones above 14; 10
pixels off, the loops of clean matches no longer close and the 2 degree cut drops up to 7 of the 270 clean ones (990: 7, 1010: 2), without splitting the graph."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _rot_l1_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC, FOCAL, GUESS, NUM_BAD, MAX_OFFSET = 60, 1000.0, 1500.0, 30, 5


def _scene(out, oracle, num_bad=NUM_BAD, max_offset=MAX_OFFSET):
    """-> the set of corrupted pairs as (frame number, frame number), the number of matches"""
    from _tracks_dataset import write_tracks
    write_tracks(out, NC, 2000, max_offset=max_offset, focal=FOCAL, focal_guess=GUESS, oracle=oracle)
    rng = np.random.default_rng(21)
    perm = rng.permutation(NC)                                                     # new position of old camera
    blocks = []
    with open(os.path.join(out, "features.dat"), "rb") as f:
        for _ in range(NC):
            nf = struct.unpack("i", f.read(4))[0]; blocks.append(struct.pack("i", nf) + f.read(nf * (8 + 4 * 128)))
    inv = np.argsort(perm)                                                         # old camera at new position
    with open(os.path.join(out, "features.dat"), "wb") as f:
        for p in range(NC):
            f.write(blocks[inv[p]])
    with open(os.path.join(out, "keyframes.txt"), "w") as f:
        f.write("%d\n" % NC)
        for p in range(NC):
            f.write("%d %06d.jpg\n" % (inv[p], inv[p] + 1))                         # the frame number is the old camera
    matches = []
    with open(os.path.join(out, "matches.dat"), "rb") as f:
        nm = struct.unpack("i", f.read(4))[0]
        for _ in range(nm):
            a, b, k = struct.unpack("3i", f.read(12)); pairs = f.read(8 * k); R = np.frombuffer(f.read(72), np.float64).reshape(3, 3).T.copy()
            matches.append([a, b, k, pairs, R])
    bad = rng.choice(nm, num_bad, replace=False)
    for e in bad:
        matches[e][4] = RR._axis_kick(rng, 20.0, 170.0) @ matches[e][4]
    with open(os.path.join(out, "matches.dat"), "wb") as f:
        f.write(struct.pack("i", nm))
        for q in rng.permutation(nm):
            a, b, k, pairs, R = matches[q]
            f.write(struct.pack("3i", int(perm[a]), int(perm[b]), k) + pairs + np.ascontiguousarray(R.T).tobytes())
    return {(matches[e][0], matches[e][1]) for e in bad}, nm


def _run(exe, out, *flags, env=None):
    res = subprocess.run([exe, "-output", out, "-width", "1920", "-height", "1080", "-seed", "3", "-viewgraph", *flags], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **(env or {})))
    focal = [float(m) for m in re.findall(r"after optimization: (\S+)", res.stdout)]
    return res, (focal[-1] if focal else None)


def _everything(res, out):
    """What a run leaves behind: its exit code, its standard output without the one timing field (SfM::Optimize prints "solve %.3f s"), and every file under the
    output directory byte for byte (costs.txt, poses.txt, calib.txt, the OBJ files, the three COLMAP models; the input files and the rotinit.txt of the L1 run
    before it lie there too and are the same for both runs)."""
    files = {}
    for d, _, names in os.walk(out):
        for name in names:
            with open(os.path.join(d, name), "rb") as f:
                files[os.path.relpath(os.path.join(d, name), out)] = f.read()
    return res.returncode, re.sub(r"solve \S+ s", "solve", res.stdout), files


def test_uncalibrated_driver_with_rotinit_l1(oracle, tmp_path):
    exe = os.path.join(ROOT, "spherical_sfm_amd", "run_spherical_sfm_uncalib")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    out = str(tmp_path / "run")
    corrupted, nm = _scene(out, oracle)
    assert len(corrupted) == NUM_BAD and nm == MAX_OFFSET * NC

    run, focal_l1 = _run(exe, out, "-rotinit", "l1")
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    line = [l for l in run.stdout.splitlines() if l.startswith("ROTINIT_RESULT")]
    assert len(line) == 1, run.stdout[-3000:]
    r = dict(kv.split("=") for kv in line[0].split()[1:])
    print(line[0])
    log = {}
    with open(os.path.join(out, "rotinit.txt")) as f:
        for l in f:
            a, b, deg, kept = l.split(); log[(int(a), int(b))] = (float(deg), int(kept))
    clean = [v for e, v in log.items() if e not in corrupted]
    print("largest clean residual [deg]:", max(v[0] for v in clean), " smallest corrupted:", min(log[e][0] for e in corrupted))
    assert len(log) == nm == int(r["edges_in"]) and int(r["cameras_in"]) == NC
    assert abs(float(r["focal_search_l1"]) - FOCAL) < 10.0                          # the search itself, before the joint refinement (docstring)
    assert all(log[e][1] == 0 for e in corrupted)                                   # the cut removes every corrupted match ...
    assert sum(1 for _, k in clean if k == 0) <= 7                                  # ... and of the clean ones no more than the restatement drops 10 pixels off
    assert int(r["edges_kept"]) == sum(k for _, k in log.values()) and int(r["cameras_kept"]) == NC and int(r["iterations"]) >= 1
    pipe = [l for l in run.stdout.splitlines() if l.startswith("PIPELINE_RESULT")][0]
    p = dict(kv.split("=") for kv in pipe.split()[1:])
    print(pipe)
    assert p["ok"] == "1111" and p["cameras"] == str(NC) and float(p["focal_guess"]) == GUESS
    assert abs(float(p["focal_search"]) - focal_l1) <= 1e-5 * focal_l1              # "after optimization" is printed with six significant digits
    assert abs(focal_l1 - FOCAL) < 80.0                                             # the bounds of the existing uncalibrated driver tests
    assert abs(float(p["focal_spherical"]) - FOCAL) < 2.0 and abs(float(p["focal_final"]) - FOCAL) < 2.0
    assert "PAIRWISE_RESULT pairs=%d " % int(r["edges_kept"]) in run.stdout

    # The same files through the tree search: its refined focal ends at the lower bound of the range, 375
    tree, focal_tree = _tree_and_no_flag(exe, out)
    got = focal_tree if focal_tree is not None else float(re.findall(r"before optimization: (\S+)", tree.stdout)[0])
    assert abs(focal_l1 - FOCAL) < abs(got - FOCAL)


def _tree_and_no_flag(exe, out, *more):
    """The files of `out` through the tree search, with "-rotinit tree" and without any flag: one and the same run, from the first line of output to the last
    pose.  Two processes are compared byte for byte through the bundle adjustments, so both run with SSFM_DETERMINISTIC=1, the library's mode for bit-identical
    repeats, as in tests/test_cpp_shim_front_gpu.py; everything before the bundle adjustment repeats bit for bit in either mode."""
    det = dict(SSFM_DETERMINISTIC="1")
    tree, focal_tree = _run(exe, out, *more, "-rotinit", "tree", env=det)
    all_tree = _everything(tree, out)
    none, focal_none = _run(exe, out, *more, env=det)
    all_none = _everything(none, out)
    before = lambda text: re.findall(r"before optimization: (\S+)", text)
    print("tree: search", before(tree.stdout), "refined", focal_tree, "; no flag: search", before(none.stdout), "refined", focal_none, "; exit codes", tree.returncode,
          none.returncode, "; files compared", sorted(all_tree[2]))
    assert "ROTINIT_RESULT" not in tree.stdout and "ROTINIT_RESULT" not in none.stdout
    assert len(all_tree[2]["costs.txt"].splitlines()) == 1024 and len(before(tree.stdout)) == 1
    assert all_tree[0] == all_none[0]
    assert all_tree[1] == all_none[1]
    assert sorted(all_tree[2]) == sorted(all_none[2])
    differ = [name for name in all_tree[2] if all_tree[2][name] != all_none[2][name]]
    assert not differ, differ
    return tree, focal_tree


def test_without_the_flag_nothing_changes_where_the_bundle_adjustments_run(oracle, tmp_path):
    """On the scene above the tree search ends at the lower bound of the range and the bundle adjustments find no camera to add, so the comparison there stops
    short of them.  The same scene without a corrupted match: the tree search is right, all four bundle adjustments of -generalba
    run, and the two runs are compared down to the poses.  Bounds of tests/test_view_graph_gpu.py::test_uncalibrated_driver_with_viewgraph_recovers_the_focal."""
    exe = os.path.join(ROOT, "spherical_sfm_amd", "run_spherical_sfm_uncalib")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    out = str(tmp_path / "run")
    corrupted, nm = _scene(out, oracle, num_bad=0)
    assert not corrupted and nm == MAX_OFFSET * NC
    tree, focal_tree = _tree_and_no_flag(exe, out, "-generalba")
    assert tree.returncode == 0, tree.stdout[-3000:] + tree.stderr[-3000:]
    pipe = [l for l in tree.stdout.splitlines() if l.startswith("PIPELINE_RESULT")][0]
    p = dict(kv.split("=") for kv in pipe.split()[1:])
    print(pipe)
    assert p["ok"] == "1111" and p["cameras"] == str(NC) and int(p["residuals"]) > 0
    assert abs(float(p["focal_search"]) - FOCAL) < 80.0 and abs(float(p["focal_spherical"]) - FOCAL) < 2.0 and abs(float(p["focal_final"]) - FOCAL) < 2.0
