"""The C++ mirror of the five-point pairwise stage on the GPU: estimate_pairwise_five_point (shim/tools.h) through demo_match on a 6-frame features.dat against
the Python call on the same match lists, and run_spherical_sfm_uncalib -match -fivepoint from keyframes.txt + features.dat to poses.txt."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _front_scene as S
import _match_ref as MR
from spherical_sfm_amd import ransac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(outdir, frames, indices=None, shift=(0.0, 0.0)):
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


def _exe(name):
    exe = os.path.join(ROOT, "spherical_sfm_amd", name)
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    return exe


def test_estimate_pairwise_five_point_mirror_equals_the_python_call(gpu_ctx, tmp_path):
    MIN = 10
    frames = S.arc_frames((130, 70, 130, 2, 0, 70), dim=128, seed=5)
    out = str(tmp_path / "m"); _write(out, frames, indices=[3, 7, 8, 20, 21, 40])
    res = subprocess.run([_exe("demo_match"), out, "%.17g" % S.FOCAL, "%.17g" % S.CX, "%.17g" % S.CY, "2", str(MIN)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("DEMO_FIVEPOINT_RESULT")]
    assert len(line) == 1, res.stdout[-2000:]
    # the Python call on the same lists: candidates are the pairs with at least MIN matches, in (index0, index1) order
    pairs = MR.exhaustive_pairs(len(frames))
    mp, m0, m1 = MR.match_pairs([f[1] for f in frames], pairs)
    cand = [k for k in range(len(pairs)) if mp[k + 1] - mp[k] >= MIN and mp[k + 1] > mp[k]]
    kinv = 1.0 / S.FOCAL
    rays = [np.c_[(np.asarray(xy, np.float32).astype(np.float64).reshape(-1, 2) - [S.CX, S.CY]) * kinv, np.ones(len(xy))] for xy, _ in frames]
    feat_ptr = np.cumsum([0] + [len(r) for r in rays]); feat_rays = np.concatenate([r.reshape(-1, 3) for r in rays])
    mptr = np.cumsum([0] + [mp[k + 1] - mp[k] for k in cand])
    i0 = np.concatenate([m0[mp[k]:mp[k + 1]] for k in cand]); i1 = np.concatenate([m1[mp[k]:mp[k + 1]] for k in cand])
    sq = (2.0 * 2.0) * kinv * kinv
    py = ransac.ransac5_batch_indexed(gpu_ctx, feat_ptr, feat_rays, [pairs[k][0] for k in cand], [pairs[k][1] for k in cand], mptr, i0, i1, sq, min_num_inliers=MIN)
    want = []
    for c, k in enumerate(cand):
        if not py["num_inliers"][c] > MIN: continue
        m = py["mask"][mptr[c]:mptr[c + 1]].astype(bool)
        want.append((pairs[k][0], pairs[k][1], list(zip(i0[mptr[c]:mptr[c + 1]][m], i1[mptr[c]:mptr[c + 1]][m])), py["R"][c]))
    got = [l.split() for l in open(os.path.join(out, "five_point.txt")).read().splitlines()]
    assert len(got) == len(want) >= 3 and ("accepted=%d" % len(want)) in line[0]
    for g, (a, b, lst, R) in zip(got, want):
        n = int(g[2])
        assert (int(g[0]), int(g[1]), n) == (a, b, len(lst))
        assert [(int(g[3 + 2 * q]), int(g[4 + 2 * q])) for q in range(n)] == [(int(j), int(i)) for j, i in lst]
        assert np.array_equal(np.array([float(x) for x in g[3 + 2 * n:]]).reshape(3, 3).T, R)           # column-major in the file; the same device call: bit for bit


def test_uncalibrated_driver_with_match_and_fivepoint_runs_to_poses(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    frames = S.ring_frames(12, per_cam=60, stray=False)
    # the driver guesses focal = (width + height) / 2 and the centre (width / 2, height / 2): 640 x 560 -> 600 and (320, 280), the scene's focal with its centre moved there
    out = str(tmp_path / "run"); _write(out, frames, shift=(320.0 - S.CX, 280.0 - S.CY))
    res = subprocess.run([_exe("run_spherical_sfm_uncalib"), "-output", out, "-width", "640", "-height", "560", "-match", "-fivepoint", "-inlierthresh", "2", "-mininliers", "20",
                          "-seed", "3"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    pw = [l for l in res.stdout.splitlines() if l.startswith("PAIRWISE_RESULT")][0]
    kv = dict(x.split("=") for x in pw.split()[1:])
    assert int(kv["pairs"]) >= 12 and int(kv["loop_closures"]) >= 1
    poses = np.loadtxt(os.path.join(out, "poses.txt"))
    assert poses.shape[0] == 12 and np.isfinite(poses).all()
