"""The view-graph calls on the device against tests/_view_graph_ref.py: ssfm_triplet_filter (filter_image_matches, examples/spherical_sfm_tools.cpp:1031-1082, both
product orders), ssfm_focal_search_graph (loop_constraint_cost_fn with the spanning tree in place of the chain) and the two drivers with -viewgraph on frames
whose file order is not the capture order.  tests/test_view_graph_cpu.py guards the fixtures: no triplet error within 1e-6 rad of the threshold."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from spherical_sfm_amd import _lib, rotavg, view_graph
from spherical_sfm_amd._lib import c_double_p, c_i32_p, c_u8_p

import _front_scene as S
import _view_graph_ref as VR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_against_reference(gpu_ctx, oracle, name, fx, order):
    n, i0, i1, R = fx[:4]
    want_good, want_count, want_tri, want_err = VR.reference_result(oracle, name, order)
    good, count, tri, err = view_graph.triplet_filter(gpu_ctx, n, i0, i1, R, VR.THRESH, order, max_records=want_count + 5)
    print(f"{name} order={order}: good {good.sum()}/{len(good)} triplets {count} max |err - ref| = {np.abs(err - want_err).max() if len(err) == len(want_err) else None}")
    assert count == want_count
    assert np.array_equal(good, want_good)
    assert np.array_equal(tri, want_tri)
    assert np.abs(err - want_err).max() <= 1e-10
    return good


def test_complete_graph_composed_order_exact_flags(gpu_ctx, oracle):
    fx = VR.complete_graph()
    good = _check_against_reference(gpu_ctx, oracle, "complete", fx, VR.ORDER_COMPOSED)
    assert len(good) == 66 and not good[fx[4]].any()                              # the six corrupted edges are in no consistent triangle


def test_complete_graph_reference_order_keeps_fewer_edges(gpu_ctx, oracle):
    """The reference multiplies Rij Rjk; with R_b = R_ab R_a a consistent triangle satisfies Rik = Rjk Rij.  On non-coaxial rotations the reference's order rejects
    consistent triangles: strictly fewer edges survive (the CPU test confirms the inequality with the reference loop alone)."""
    fx = VR.complete_graph()
    good_ref = _check_against_reference(gpu_ctx, oracle, "complete", fx, VR.ORDER_REFERENCE)
    good_cmp = view_graph.triplet_filter(gpu_ctx, fx[0], fx[1], fx[2], fx[3], VR.THRESH, VR.ORDER_COMPOSED)[0]
    assert good_ref.sum() < good_cmp.sum()


def test_ring_reference_order_keeps_every_clean_edge(gpu_ctx, oracle):
    fx = VR.ring(oracle)
    good = _check_against_reference(gpu_ctx, oracle, "ring", fx, VR.ORDER_REFERENCE)
    assert good[np.setdiff1d(np.arange(len(good)), fx[4])].all()


def _raw_call(ctx, n, i0, i1, R, max_records, tri, err, good, order=VR.ORDER_COMPOSED):
    rel = np.ascontiguousarray(np.transpose(R, (0, 2, 1))).reshape(-1).copy(); nt = C.c_int64(-1)
    rc = _lib.lib().ssfm_triplet_filter(ctx._p, n, len(i0), i0.ctypes.data_as(c_i32_p), i1.ctypes.data_as(c_i32_p), rel.ctypes.data_as(c_double_p), float(VR.THRESH), order,
                                        good.ctypes.data_as(c_u8_p), C.byref(nt), max_records, tri.ctypes.data_as(c_i32_p), err.ctypes.data_as(c_double_p))
    return rc, nt.value


def test_edge_cases_in_one_list(gpu_ctx, oracle, monkeypatch):
    """Unsorted, duplicates, a self loop, edges stored (b, a), out-degree 70 (> one wave) and 0; max_records below the count; no edges; an index out of range."""
    fx = VR.edge_cases()
    n, i0, i1, R = fx
    for order in (VR.ORDER_REFERENCE, VR.ORDER_COMPOSED):
        _check_against_reference(gpu_ctx, oracle, "edge_cases", fx, order)
    want_good, count, want_tri, want_err = VR.reference_result(oracle, "edge_cases", VR.ORDER_COMPOSED)
    # fewer records than triplets: exactly the first ones, nothing past the end (canaries behind both buffers)
    m = count // 2; assert 0 < m < count
    tri = np.full(3 * m + 12, -77, np.int32); err = np.full(m + 4, -77.0); good = np.zeros(len(i0), np.uint8)
    rc, nt = _raw_call(gpu_ctx, n, i0, i1, R, m, tri, err, good)
    assert rc == 0 and nt == count and np.array_equal(good.astype(bool), want_good)
    assert np.array_equal(tri[:3 * m].reshape(-1, 3), want_tri[:m]) and np.abs(err[:m] - want_err[:m]).max() <= 1e-10
    assert (tri[3 * m:] == -77).all() and (err[m:] == -77.0).all()
    # the same records through many slabs: 3 records per slab -- the first edge (75, 0) alone has 5 triplets and gets a slab of its own, larger than the bound; the cut
    # at max_records falls inside a slab
    monkeypatch.setenv("SSFM_TRIPLET_SLAB_RECORDS", "3")
    for mm in (count + 5, m):
        tri = np.full(3 * mm + 12, -77, np.int32); err = np.full(mm + 4, -77.0)
        rc, nt = _raw_call(gpu_ctx, n, i0, i1, R, mm, tri, err, good)
        k = min(mm, count)
        assert rc == 0 and nt == count and np.array_equal(tri[:3 * k].reshape(-1, 3), want_tri[:k]) and np.abs(err[:k] - want_err[:k]).max() <= 1e-10
        assert (tri[3 * k:] == -77).all() and (err[k:] == -77.0).all()
    monkeypatch.delenv("SSFM_TRIPLET_SLAB_RECORDS")
    # no edges: valid, zero triplets
    good, nt = view_graph.triplet_filter(gpu_ctx, 5, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 3, 3)), VR.THRESH)
    assert len(good) == 0 and nt == 0
    # an index out of range: refused (on the host, before any launch -- the CPU test shows the check precedes the look at the context), outputs untouched
    bad0 = i0.copy(); bad0[17] = n
    good = np.full(len(i0), 9, np.uint8)
    rc, nt = _raw_call(gpu_ctx, n, bad0, i1, R, m, tri, err, good)
    assert rc == -1 and b"out of range" in _lib.lib().ssfm_last_error(gpu_ctx._p) and (good == 9).all() and nt == -1
    bad1 = i1.copy(); bad1[3] = -1
    with pytest.raises(_lib.SsfmError, match="out of range"):
        view_graph.triplet_filter(gpu_ctx, n, i0, bad1, R, VR.THRESH)


def test_repeat_is_bit_identical(gpu_ctx):
    n, i0, i1, R, _ = VR.complete_graph()
    a = view_graph.triplet_filter(gpu_ctx, n, i0, i1, R, VR.THRESH, VR.ORDER_COMPOSED, max_records=300)
    b = view_graph.triplet_filter(gpu_ctx, n, i0, i1, R, VR.THRESH, VR.ORDER_COMPOSED, max_records=300)
    assert a[1] == b[1] == 220 and all(x.tobytes() == y.tobytes() for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])))


def test_focal_search_graph_matches_the_oracle(gpu_ctx, oracle):
    """The ring of the filter test with its 4 corrupted edges, edge list shuffled, cameras renumbered: no chain exists.  Tolerances of tests/test_focal_search_gpu.py."""
    n, i0, i1, R_rel, perm = VR.shuffled_ring(oracle)
    focals = np.random.default_rng(3).uniform(1300.0 / 4, 1300.0 * 2, 48)
    root = 0
    costs, best, rot = view_graph.focal_search_graph(gpu_ctx, n, i0, i1, R_rel, 1300.0, focals, root=root)
    ref = []; rots = []
    for f in focals:
        c, r = VR.oracle_cost_tree(oracle, n, i0, i1, R_rel, f, 1300.0, root)
        ref.append(c); rots.append(r)
    ref = np.array(ref)
    print("focal_search_graph: max |cost - ref| / max ref =", np.abs(costs - ref).max() / ref.max(), "rot", np.abs(rot - rots[best]).max(), "best focal", focals[best])
    assert np.abs(costs - ref).max() <= 1e-9 * ref.max()
    assert best == int(np.argmin(ref))
    assert np.abs(rot - rots[best]).max() < 1e-10
    assert abs(focals[best] - 1000.0) < 0.08 * 1000.0
    # another root: another tree, the same agreement
    costs2, best2, rot2 = view_graph.focal_search_graph(gpu_ctx, n, i0, i1, R_rel, 1300.0, focals[:4], root=17)
    for t in range(4):
        c, r = VR.oracle_cost_tree(oracle, n, i0, i1, R_rel, focals[t], 1300.0, 17)
        assert abs(costs2[t] - c) <= 1e-9 * ref.max()
    assert np.array_equal(rot2[17], np.eye(3))


def test_chain_through_the_graph_variant(gpu_ctx, oracle):
    """On a pure chain (edges (k-1, k) only, root 0) the tree is the chain: focal_search_graph must give what focal_search gives."""
    from _uncalib_graph import make_uncalibrated_loop
    i0, i1, R_rel, _ = make_uncalibrated_loop(oracle, 40, 3, focal_true=1000.0, focal_guess=1300.0)
    keep = i1 == i0 + 1
    i0, i1, R_rel = i0[keep], i1[keep], R_rel[keep]
    assert len(i0) == 39
    focals = np.random.default_rng(3).uniform(1300.0 / 4, 1300.0 * 2, 48)
    ca, ba_, ra = rotavg.focal_search(gpu_ctx, 40, i0, i1, R_rel, 1300.0, focals)
    cb, bb, rb = view_graph.focal_search_graph(gpu_ctx, 40, i0, i1, R_rel, 1300.0, focals, root=0)
    print("chain: rot diff", np.abs(ra - rb).max(), "cost diff", np.abs(ca - cb).max(), "cost max", ca.max())
    assert np.abs(ra - rb).max() <= 1e-12 and (np.abs(ca - cb) <= 1e-12 * ca).all() and ba_ == bb


# ---- drivers -------------------------------------------------------------------------------------------------------------------------------------------------------

def _exe(name):
    exe = os.path.join(ROOT, "spherical_sfm_amd", name)
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    return exe


def _write_features(outdir, frames, indices):
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
    with open(os.path.join(outdir, "intrinsics.txt"), "w") as f:
        f.write("%.17g %.17g %.17g\n" % (S.FOCAL, S.CX, S.CY))


def _max_rotation_error_deg(outdir, num):
    """poses.txt against the ring's ground truth R_i = so3exp((0, 2 pi i / num, 0)), after the one global rotation that aligns them best"""
    from scipy.spatial.transform import Rotation
    poses = np.loadtxt(os.path.join(outdir, "poses.txt"))
    ids = poses[:, 0].astype(int)
    Rs = Rotation.from_rotvec(poses[:, 4:7]).as_matrix()
    Rgt = Rotation.from_rotvec(np.stack([np.zeros(len(ids)), 2 * np.pi * ids / num, np.zeros(len(ids))], axis=1)).as_matrix()
    U, _, Vt = np.linalg.svd(sum(Rgt[k].T @ Rs[k] for k in range(len(ids))))      # R_est = R_gt G: the G closest to every R_gt^T R_est
    G = U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt
    err = [np.linalg.norm(Rotation.from_matrix(Rs[k] @ (Rgt[k] @ G).T).as_rotvec()) for k in range(len(ids))]
    return ids, float(np.rad2deg(max(err)))


def test_calibrated_driver_with_viewgraph_on_shuffled_frames(tmp_path):
    """12 ring frames + 2 stray ones, written in a shuffled order (keyframes.txt keeps the capture numbers): run_spherical_sfm -match -viewgraph must reconstruct the
    ring as well as the existing -match run does from the capture order (the parent's behaviour, measured here on the same frames)."""
    exe = _exe("run_spherical_sfm")
    N = 12
    frames = S.ring_frames(N, 60, stray=True)
    order = np.random.default_rng(6).permutation(len(frames))
    assert not np.array_equal(order, np.arange(len(frames)))
    errs = {}
    for tag, idx, flags in (("capture", np.arange(len(frames)), ["-match"]), ("shuffled", order, ["-match", "-viewgraph"])):
        out = str(tmp_path / tag)
        _write_features(out, [frames[i] for i in idx], [int(i) for i in idx])
        res = subprocess.run([exe, "-intrinsics", os.path.join(out, "intrinsics.txt"), "-output", out, "-inlierthresh", "2", "-mininliers", "20", *flags],
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        ids, errs[tag] = _max_rotation_error_deg(out, N)
        assert sorted(ids.tolist()) == list(range(N)), ids                        # the 12 ring frames are kept, the stray pair is gone
        if tag == "shuffled":
            assert "good edges" in res.stdout
    print("max rotation error [deg]: capture order, sequential:", errs["capture"], " shuffled, -viewgraph:", errs["shuffled"])
    # Both runs end in the same bundle adjustments of the same tracks; what differs is the start (another spanning tree, another gauge camera), so they reach the
    # same minimum up to the solver's tolerances.  Measured once on an MI355X: capture order 0.0515310 deg, shuffled with -viewgraph 0.0515352 deg, a difference of
    # 4.2e-6 deg.  The margin allows a fifth of the noise-level error itself; a start that sent the adjustment elsewhere would miss by degrees.
    margin_deg = 0.01
    assert errs["shuffled"] <= errs["capture"] + margin_deg


def test_uncalibrated_driver_with_viewgraph_recovers_the_focal(oracle, tmp_path):
    """run_spherical_sfm_uncalib -viewgraph on feature tracks (tests/_tracks_dataset.py, as tests/test_cpp_shim_gpu.py writes them: matches estimated at the guessed
    focal 1500, true focal 1000) whose cameras are renumbered by a random permutation and whose match list is shuffled: no chain exists.  Bounds of the existing
    sequential driver test."""
    from _tracks_dataset import write_tracks
    exe = _exe("run_spherical_sfm_uncalib")
    out = str(tmp_path / "run"); Nc, Np = 60, 2000
    write_tracks(out, Nc, Np, focal=1000.0, focal_guess=1500.0, oracle=oracle)
    rng = np.random.default_rng(12)
    perm = rng.permutation(Nc)                                                    # new position of old camera
    # features.dat: per-frame blocks in the new order
    blocks = []
    with open(os.path.join(out, "features.dat"), "rb") as f:
        for _ in range(Nc):
            nf = struct.unpack("i", f.read(4))[0]; blocks.append(struct.pack("i", nf) + f.read(nf * (8 + 4 * 128)))
    inv = np.argsort(perm)                                                        # old camera at new position
    with open(os.path.join(out, "features.dat"), "wb") as f:
        for p in range(Nc):
            f.write(blocks[inv[p]])
    with open(os.path.join(out, "keyframes.txt"), "w") as f:
        f.write("%d\n" % Nc)
        for p in range(Nc):
            f.write("%d %06d.jpg\n" % (inv[p], inv[p] + 1))
    matches = []
    with open(os.path.join(out, "matches.dat"), "rb") as f:
        nm = struct.unpack("i", f.read(4))[0]
        for _ in range(nm):
            a, b, k = struct.unpack("3i", f.read(12)); matches.append((int(perm[a]), int(perm[b]), k, f.read(8 * k + 72)))
    with open(os.path.join(out, "matches.dat"), "wb") as f:
        f.write(struct.pack("i", nm))
        for q in rng.permutation(nm):
            a, b, k, rest = matches[q]; f.write(struct.pack("3i", a, b, k) + rest)
    res = subprocess.run([exe, "-output", out, "-width", "1920", "-height", "1080", "-generalba", "-seed", "3", "-viewgraph"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("PIPELINE_RESULT")][0]
    r = dict(kv.split("=") for kv in line.split()[1:])
    print(line)
    assert r["ok"] == "1111" and float(r["focal_guess"]) == 1500.0 and r["cameras"] == str(Nc)
    assert abs(float(r["focal_search"]) - 1000.0) < 80.0
    assert abs(float(r["focal_spherical"]) - 1000.0) < 2.0 and abs(float(r["focal_final"]) - 1000.0) < 2.0
