"""CPU side of the view-graph calls (ssfm_triplet_filter, ssfm_view_graph_tree, ssfm_focal_search_graph): the spanning tree against a Python BFS, the chaining it
feeds, the refusals that come before a context is looked at, the condition on the GPU test's fixtures, the resources of the three kernels read from the built
code object, and the host code (CSR sort, tree, join, the mirror's bookkeeping) in a stand-alone program under ASan + UBSan.  No kernel is launched here."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from spherical_sfm_amd import _lib, synth, view_graph

import _view_graph_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIB = os.path.join(ROOT, "spherical_sfm_amd", "libssfm_hip.so")
TREE_KEYS = ("node", "parent", "edge", "reversed", "level_ptr")


def _random_graph(rng, t):
    """2-25 nodes; disconnected parts, duplicates, self loops and edges in both directions come with the draw, zero edges and root != 0 by construction"""
    n = int(rng.integers(2, 26))
    E = 0 if t % 10 == 0 else int(rng.integers(1, 3 * n))
    span = n if t % 3 else max(1, n // 2)                                         # every third graph leaves half of its nodes without an edge
    i0 = rng.integers(0, span, E).astype(np.int32); i1 = rng.integers(0, span, E).astype(np.int32)
    if E > 4:
        i0[1], i1[1] = i0[0], i1[0]                                               # a duplicate
        i1[2] = i0[2]                                                             # a self loop
        i0[3], i1[3] = i1[0], i0[0]                                               # the first edge again, stored the other way round
    root = 0 if t % 4 == 0 else int(rng.integers(0, n))
    return n, i0, i1, root


def test_tree_equals_the_python_bfs():
    rng = np.random.default_rng(21)
    shapes = set()
    for t in range(30):
        n, i0, i1, root = _random_graph(rng, t)
        got = view_graph.spanning_tree(n, i0, i1, root); want = VR.bfs_tree(n, i0, i1, root)
        assert (got["num_reached"], got["num_levels"]) == (want["num_reached"], want["num_levels"]), (t, got, want)
        for k in TREE_KEYS:
            assert np.array_equal(got[k], want[k]), (t, k, got[k], want[k])
        assert got["node"][0] == root and got["parent"][0] == -1 and got["edge"][0] == -1
        shapes.add((len(i0) == 0, root != 0, got["num_reached"] < n, bool(got["reversed"].any())))
    assert {s[0] for s in shapes} == {True, False} and {s[1] for s in shapes} == {True, False} and {s[2] for s in shapes} == {True, False} and any(s[3] for s in shapes)


def test_tree_refuses_bad_roots_and_indices():
    for n, i0, i1, root in ((3, [0, 3], [1, 1], 0), (3, [0, 1], [1, -1], 0), (3, [0], [1], 3), (3, [0], [1], -1), (0, [], [], 0)):
        with pytest.raises(_lib.SsfmError, match="out of range"):
            view_graph.spanning_tree(n, np.array(i0, np.int32), np.array(i1, np.int32), root)


def test_chaining_a_noise_free_graph_reproduces_its_rotations():
    rng = np.random.default_rng(8)
    for t in range(5):
        n = int(rng.integers(5, 26))
        R_gt = synth.so3exp(rng.normal(size=(n, 3)) * 0.7)
        # connected: a random spanning tree in random directions plus extra edges, shuffled
        pairs = [(int(rng.integers(0, k)), k) for k in range(1, n)] + [tuple(rng.integers(0, n, 2)) for _ in range(n)]
        pairs = [(b, a) if rng.random() < 0.5 else (a, b) for a, b in pairs]
        pairs = [pairs[k] for k in rng.permutation(len(pairs))]
        i0, i1 = np.array(pairs, np.int32).T
        rel = np.stack([R_gt[b] @ R_gt[a].T for a, b in pairs])
        root = int(rng.integers(0, n))
        rot = view_graph.initialize_rotations_tree(n, i0, i1, rel, root)
        assert np.abs(rot - R_gt @ R_gt[root].T).max() <= 1e-12                    # up to the root's rotation
        assert np.array_equal(rot, VR.chain_tree(n, VR.bfs_tree(n, i0, i1, root), rel))


def test_symbols_and_refusals_before_any_launch():
    L = _lib.lib()
    for s in ("ssfm_triplet_filter", "ssfm_view_graph_tree", "ssfm_focal_search_graph"):
        assert hasattr(L, s) and s in _lib.DECLARED_SYMBOLS
    R = np.tile(np.eye(3), (2, 1, 1))
    # an index out of range is found on the host, before the (missing) context is looked at: nothing can have been launched
    for i0, i1 in (([0, 3], [1, 1]), ([0, 1], [1, -1])):
        with pytest.raises(_lib.SsfmError, match="camera index out of range"):
            view_graph.triplet_filter(None, 3, np.array(i0, np.int32), np.array(i1, np.int32), R, 0.1)
    with pytest.raises(_lib.SsfmError, match="bad arguments"):
        view_graph.triplet_filter(None, 3, np.array([0, 1], np.int32), np.array([1, 2], np.int32), R, 0.1, order=2)
    with pytest.raises(_lib.SsfmError, match="ctx is null"):
        view_graph.triplet_filter(None, 3, np.array([0, 1], np.int32), np.array([1, 2], np.int32), R, 0.1)


@pytest.mark.parametrize("name", ["complete", "ring", "edge_cases"])
def test_fixture_guard_no_triplet_error_near_the_threshold(oracle, name):
    """A condition on the INPUTS of tests/test_view_graph_gpu.py, checked with the reference loop alone: no triplet error lies within 1e-6 rad of the threshold, so
    the exact comparison of the flags there cannot rest on last bits."""
    for order in (VR.ORDER_REFERENCE, VR.ORDER_COMPOSED):
        good, count, tri, err = VR.reference_result(oracle, name, order)
        assert count > 0 and np.abs(err - VR.THRESH).min() > 1e-6, (name, order, np.abs(err - VR.THRESH).min())
        assert (err < VR.THRESH).any() and (err >= VR.THRESH).any()                # both sides of the threshold occur


def test_fixtures_are_what_the_gpu_tests_assume(oracle):
    n, i0, i1, R, bad = VR.complete_graph()
    assert (n, len(i0)) == (12, 66) and VR.reference_result(oracle, "complete", VR.ORDER_COMPOSED)[1] == 220
    # the finding: the reference's product order keeps strictly fewer edges of a consistent non-coaxial graph than the order the edge convention implies
    assert VR.reference_result(oracle, "complete", VR.ORDER_REFERENCE)[0].sum() < VR.reference_result(oracle, "complete", VR.ORDER_COMPOSED)[0].sum()
    assert not VR.reference_result(oracle, "complete", VR.ORDER_COMPOSED)[0][bad].any()
    n, i0, i1, R, bad = VR.ring(oracle)
    good = VR.reference_result(oracle, "ring", VR.ORDER_REFERENCE)[0]
    assert good[np.setdiff1d(np.arange(len(i0)), bad)].all() and not good[bad].any()
    n, i0, i1, R = VR.edge_cases()
    assert np.bincount(i0, minlength=n).max() >= 70 and np.bincount(i0, minlength=n)[79] == 0 and (i0 == i1).any() and (i0 > i1).sum() >= 2
    assert len(set(zip(i0.tolist(), i1.tolist()))) < len(i0) and not np.array_equal(np.lexsort((i1, i0)), np.arange(len(i0)))
    n, s0, s1, Rs, perm = VR.shuffled_ring(oracle)
    assert not any(((s0 == k - 1) & (s1 == k)).any() for k in range(1, 4))         # no chain to follow


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(KR.READELF)), reason="needs the built library and llvm-readelf")
def test_view_graph_kernels_have_no_spills_and_no_dynamic_stack():
    ks = {k["short"]: k for k in KR.kernels(LIB).values()}
    for want in ("k_triplet_filter", "k_triplet_records", "k_focal_trials_graph"):
        names = [n for n in ks if n.startswith(want) or ("::" + want) in n]
        assert names, (want, [n for n in ks if "triplet" in n or "graph" in n])
        for n in names:
            # the trial kernel shares its body with k_focal_trials, whose essential-matrix decomposition keeps a small indexed array in scratch: no more than that one
            allowed = ks["k_focal_trials"]["scratch"] if want == "k_focal_trials_graph" else 0
            assert ks[n]["scratch"] <= allowed and ks[n]["vgpr_spill"] == 0 and not ks[n]["dynamic_stack"], ks[n]


def test_host_code_under_sanitizers(tmp_path):
    """tests/native/view_graph_check.cpp: the CSR sort, the two bounds of the join, the tree builder, the join itself against the reference's triple loop and the
    mirror's apply_triplet_filter on hand-made and random multigraphs.  ASan + UBSan, host objects only."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "view_graph_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "view_graph_check.cpp"),
                         os.path.join(ROOT, "spherical_sfm_amd", "csrc", "shim", "tools_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "VIEW_GRAPH_CHECK ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr
