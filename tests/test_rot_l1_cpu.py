"""CPU side of ssfm_rot_l1_init: the condition on the fixtures of tests/test_rot_l1_gpu.py (checked with the dense numpy restatement alone), the floor under that
file's parity tolerance (dense solve against conjugate gradients at 1e-10, both in numpy), the refusals that come before a context is looked at, the resources of
the five kernels read from the built code object, and the host helpers (argument checks, reach set, adjacency) in a stand-alone program under ASan + UBSan.
No kernel is launched here.

Figures of the ring60 fixtures (numpy restatement, defaults, root 0), seeds 0-9 tried, the GPU tests use 0 and 4:
  seed  tree start max / median   L1 start max   outer iterations   corrupted kept / clean dropped by the 2 degree cut
   0      177.7 / 0.6 deg           0.368 deg          18                 0 / 0
   4      164.4 / 26.6 deg          0.350 deg          19                 0 / 0      <- the wrong-subtree seed
  (seeds 1-3, 5-9: L1 start 0.38-0.62 deg, no edge on the wrong side of the cut, but a tree median below 1.2 deg)
Dense against PCG(1e-10) on those two seeds: at most 8.8e-12 rad after 5 iterations, 1.1e-14 after 20."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from spherical_sfm_amd import _lib, view_graph

import _rot_l1_ref as RR
import _view_graph_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIB = os.path.join(ROOT, "spherical_sfm_amd", "libssfm_hip.so")
PARITY_TOL = 1e-9                 # what tests/test_rot_l1_gpu.py asserts; must stay >= 100 x the floor measured below


def test_fixture_guard_ring60():
    medians = {}
    for seed in RR.RING60_SEEDS:
        n, i0, i1, R, R_gt, bad = RR.ring60(seed)
        assert (n, len(i0), int(bad.sum())) == (60, 300, 45)
        tree = VR.chain_tree(n, VR.bfs_tree(n, i0, i1, 0), R)
        terr = RR.error_to_truth_deg(tree, R_gt, 0)
        Rl, res, s = RR.dense_result("ring60", seed, 0, 0)
        lerr = RR.error_to_truth_deg(Rl, R_gt, 0)
        keep = res <= RR.CUT
        print(f"ring60({seed}): tree max {terr.max():.1f} median {np.median(terr):.1f} deg; L1 max {lerr.max():.3f} deg after {s['iterations']} iterations; "
              f"corrupted kept {(keep & bad).sum()}, clean dropped {(~keep & ~bad).sum()}; cost {s['initial_cost']:.2f} -> {s['final_cost']:.2f}")
        assert lerr.max() <= 1.0
        assert s["termination"] == RR.CONVERGENCE and s["final_cost"] < s["initial_cost"]
        assert np.array_equal(keep, ~bad)                                          # the cut keeps no corrupted edge and drops no clean one
        # no residual within 1e-3 rad of the cut: the exact comparison of the kept set on the device cannot rest on last bits
        assert np.abs(res - RR.CUT).min() > 1e-3
        medians[seed] = float(np.median(terr))
    assert medians[RR.WRONG_SUBTREE_SEED] > 20.0, medians


def test_parity_floor_dense_against_pcg():
    """The two numpy restatements against each other: the floor under the device parity tolerance, which has to be at least 100 times above it."""
    worst = 0.0
    for seed in RR.RING60_SEEDS:
        n, i0, i1, R, _, _ = RR.ring60(seed)
        for K in (5, 20):
            A = RR.dense_result("ring60", seed, 0, K)
            B = RR.l1_irls(n, i0, i1, R, 0, "pcg", max_iterations=K, step_tolerance=0.0)
            d_rot = float(RR.geodesic(A[0], B[0]).max()); d_res = float(np.abs(A[1] - B[1]).max())
            print(f"ring60({seed}) K={K}: dense - pcg rotations {d_rot:.2e} rad residuals {d_res:.2e}; CG iterations {B[2]['pcg_iterations_total']}")
            assert A[2]["iterations"] == B[2]["iterations"] == K and B[2]["pcg_solves_capped"] == 0
            worst = max(worst, d_rot, d_res)
    assert 100.0 * worst <= PARITY_TOL, worst


def test_other_fixtures_are_what_the_gpu_tests_assume():
    n, i0, i1, R, R_gt, bad = RR.complete24()
    tree = VR.bfs_tree(n, i0, i1, 0)
    assert (n, len(i0)) == (24, 276) and bad[0] and tree["edge"][1] == 0 and 0.2 < bad.mean() < 0.3
    Rl, res, s = RR.dense_result("complete24", None, 0, 0)
    assert RR.error_to_truth_deg(Rl, R_gt, 0).max() <= 1.0 and np.array_equal(res <= RR.CUT, ~bad)
    n, i0, i1, R = RR.chain_only()
    assert len(i0) == n - 1 and VR.bfs_tree(n, i0, i1, 0)["num_reached"] == n and (i0 > i1).any()
    n, i0, i1, R, second = RR.two_components()
    t = VR.bfs_tree(n, i0, i1, 0)
    assert t["num_reached"] == 30 and second.sum() == 40 and 0 < np.flatnonzero(second)[0] < np.flatnonzero(~second)[-1]
    n, i0, i1, R = VR.edge_cases()
    assert VR.bfs_tree(n, i0, i1, 0)["num_reached"] == VR.bfs_tree(n, i0, i1, 75)["num_reached"] < n
    n, i0, i1, R, _, _ = RR.ring350()
    assert 3 * n > 1024 and len(i0) == 1750


def test_symbols_and_refusals_before_any_launch():
    L = _lib.lib()
    for sym in ("ssfm_rot_l1_default_options", "ssfm_rot_l1_init"):
        assert hasattr(L, sym) and sym in _lib.DECLARED_SYMBOLS
    o = _lib.RotL1OptionsC(); L.ssfm_rot_l1_default_options(o)
    assert {k: getattr(o, k) for k, _ in o._fields_} == RR.DEFAULTS
    R = np.tile(np.eye(3), (2, 1, 1)); i0 = np.array([0, 1], np.int32); i1 = np.array([1, 2], np.int32)
    # every refusal is made on the host before the (missing) context is looked at: nothing can have been launched
    for b0, b1 in (([0, 3], [1, 1]), ([0, 1], [1, -1])):
        with pytest.raises(_lib.SsfmError, match="camera index out of range"):
            view_graph.initialize_rotations_l1(None, 3, np.array(b0, np.int32), np.array(b1, np.int32), R)
    for root in (3, -1):
        with pytest.raises(_lib.SsfmError, match="root out of range"):
            view_graph.initialize_rotations_l1(None, 3, i0, i1, R, root=root)
    for bad in (dict(max_iterations=0), dict(weight_floor=0.0), dict(pcg_tolerance=0.0), dict(step_tolerance=-1.0), dict(pcg_max_iterations=-1),
                dict(weight_floor=float("nan"))):
        with pytest.raises(_lib.SsfmError, match="bad options"):
            view_graph.initialize_rotations_l1(None, 3, i0, i1, R, **bad)
    with pytest.raises(_lib.SsfmError, match="ctx is null"):
        view_graph.initialize_rotations_l1(None, 3, i0, i1, R)
    with pytest.raises(_lib.SsfmError, match="ctx is null"):
        view_graph.initialize_rotations_l1(None, 3, i0, i1, R, step_tolerance=0.0)    # zero is a valid step tolerance
    with pytest.raises(TypeError):
        view_graph.initialize_rotations_l1(None, 3, i0, i1, R, no_such_option=1)


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(KR.READELF)), reason="needs the built library and llvm-readelf")
def test_rot_l1_kernels_have_no_scratch_and_no_dynamic_stack():
    ks = {k["short"]: k for k in KR.kernels(LIB).values()}
    for want in ("k_l1_edges", "k_l1_nodes", "k_l1_matvec", "k_l1_cg_update", "k_l1_apply"):
        names = [n for n in ks if n.startswith(want) or ("::" + want) in n]
        assert names, (want, [n for n in ks if "l1" in n])
        if want == "k_l1_cg_update":
            assert len(names) == 2, names                                          # the start and the iteration
        for n in names:
            assert ks[n]["scratch"] == 0 and ks[n]["vgpr_spill"] == 0 and not ks[n]["dynamic_stack"], ks[n]


def test_host_helpers_under_sanitizers(tmp_path):
    """tests/native/rot_l1_host_check.cpp: rot_l1_check's refusals and their order, the reach set and the adjacency against brute force on the fixtures' shapes
    and on random multigraphs; the mirror's residual cut and its component step that carries rotations.  ASan + UBSan, host code only."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "rot_l1_host_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tests", "native", "rot_l1_host_check.cpp"), os.path.join(ROOT, "spherical_sfm_amd", "csrc", "shim", "tools_host.cpp"),
                         "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ROT_L1_HOST_CHECK ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr
