"""ssfm_focal_search_l1 on the device: parity with the composition of the existing calls it is defined by (focal_search_graph with one trial for the matches,
initialize_rotations_l1 on them with the same options), the pure chain, independence of a trial from its position, the slab and the placement, recovery of the
focal where the tree search fails, and the refusals.  tests/test_focal_l1_cpu.py guards the fixtures.

Bounds: the rotations bound is the one tests/test_rot_l1_gpu.py holds ssfm_rot_l1_init to (1e-9 rad; that file's docstring derives it); a residual depends on two
rotations (2e-9), a cost on one residual per used edge (2e-9 x used edges).  The matches and get_cost are the same device functions on the same values: 1e-12
relative, the bound of tests/test_view_graph_gpu.py::test_chain_through_the_graph_variant."""
import numpy as np
import pytest

from spherical_sfm_amd import _lib, rotavg, view_graph

import _focal_l1_ref as FR
import _rot_l1_ref as RR
import _view_graph_ref as VR

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _parity(gpu_ctx, n, i0, i1, R, focal_guess, focals, root, **opt):
    costs, best, rot_b, info = view_graph.focal_search_l1(gpu_ctx, n, i0, i1, R, focal_guess, focals, root=root, return_matches=True, **opt)
    assert best == int(np.argmin(costs)) and len(costs) == len(focals)
    for t, f in enumerate(focals):
        # the composition the call is defined by
        _, _, _, matches = view_graph.focal_search_graph(gpu_ctx, n, i0, i1, R, focal_guess, [f], root=root, return_matches=True)
        want_R, want_res, s = view_graph.initialize_rotations_l1(gpu_ctx, n, i0, i1, matches, root=root, **dict(FR.DEFAULTS, **opt))
        # the trial alone: its rotations, matches and residuals are outputs then
        c1, b1, rot, inf = view_graph.focal_search_l1(gpu_ctx, n, i0, i1, R, focal_guess, [f], root=root, return_matches=True, **opt)
        assert b1 == 0 and c1[0] == costs[t] and inf["get_costs"][0] == info["get_costs"][t] and inf["iterations"][0] == info["iterations"][t]
        used = want_res >= 0
        d_rot = float(RR.geodesic(rot, want_R).max()); d_res = float(np.abs(inf["residual"] - want_res).max()); d_cost = abs(c1[0] - s["final_cost"])
        d_rel = float(np.abs(inf["matches"] - matches).max())
        gc = rotavg.get_cost(gpu_ctx, rot, i0, i1, inf["matches"]); d_gc = abs(inf["get_costs"][0] - gc) / gc
        print(f"  focal {f:7.1f}: rotations {d_rot:.2e} rad, residuals {d_res:.2e}, cost {c1[0]:.6f} (diff {d_cost:.2e}, {used.sum()} used edges), matches {d_rel:.2e}, "
              f"get_cost {gc:.6e} (rel diff {d_gc:.2e}), iterations {inf['iterations'][0]} / {s['iterations']}, CG iterations of the composition {s['pcg_iterations_total']}")
        assert np.array_equal(inf["residual"] < 0, ~used)
        assert inf["iterations"][0] == s["iterations"]
        assert d_rot <= TOL and d_res <= 2 * TOL and d_cost <= 2 * TOL * used.sum()
        assert d_rel <= 1e-12 and d_gc <= 1e-12
        if t == best:
            assert np.array_equal(rot, rot_b) and np.array_equal(inf["residual"], info["residual"]) and np.array_equal(inf["matches"], info["matches"])
    return costs, best, rot_b, info


def test_parity_f24(gpu_ctx, oracle):
    n, i0, i1, R, _ = FR.f24(oracle)
    _, _, _, info = _parity(gpu_ctx, n, i0, i1, R, FR.FOCAL_GUESS, [700.0, 900.0, 1000.0, 1150.0, 1600.0], 0, max_iterations=3, step_tolerance=0.0)
    assert (info["iterations"] == 3).all()


def test_parity_ring350_strided_loops(gpu_ctx):
    """n = 350 > 256 lanes and E = 1750: every strided loop of the workgroup runs more than once; 16 n + 4 E doubles = 99 KiB still sit in LDS"""
    n, i0, i1, R, _, _ = RR.ring350()
    _parity(gpu_ctx, n, i0, i1, R, 1000.0, [900.0, 1100.0], 0, max_iterations=2)


@pytest.mark.parametrize("root", [0, 75])
def test_parity_edge_cases(gpu_ctx, root):
    """a node of degree 70, duplicates, a self loop, edges stored as (b, a), cameras the root does not reach"""
    n, i0, i1, R = VR.edge_cases()
    _, _, rot, info = _parity(gpu_ctx, n, i0, i1, R, 1000.0, [900.0, 1150.0], root, max_iterations=3, step_tolerance=0.0)
    reached = np.zeros(n, bool); t = VR.bfs_tree(n, i0, i1, root); reached[t["node"][:t["num_reached"]]] = True
    assert not reached.all() and (rot[~reached] == np.eye(3)).all() and np.array_equal(rot[root], np.eye(3))
    assert (info["residual"][i0 == i1] == -1).all()


def test_parity_two_components(gpu_ctx):
    n, i0, i1, R, second = RR.two_components()
    _, _, rot, info = _parity(gpu_ctx, n, i0, i1, R, 1000.0, [900.0, 1150.0], 0, max_iterations=3, step_tolerance=0.0)
    assert (info["residual"][second] == -1).all() and (info["residual"][~second] >= 0).all()
    assert (rot[30:] == np.eye(3)).all() and np.array_equal(rot[0], np.eye(3))
    # a root without used edges (camera 50 has no edge): identities, no iteration, every edge unused
    costs, best, rot, info = view_graph.focal_search_l1(gpu_ctx, n, i0, i1, R, 1000.0, [900.0, 1150.0], root=50)
    assert (costs == 0.0).all() and best == 0 and (rot == np.eye(3)).all() and (info["iterations"] == 0).all() and (info["residual"] == -1).all()


def test_pure_chain_equals_the_tree_search(gpu_ctx):
    n, i0, i1, R = RR.chain_only()
    focals = [800.0, 1000.0, 1300.0]
    costs, best, rot, info = view_graph.focal_search_l1(gpu_ctx, n, i0, i1, R, 1000.0, focals)
    for t, f in enumerate(focals):
        c, _, rot_t = view_graph.focal_search_graph(gpu_ctx, n, i0, i1, R, 1000.0, [f])
        _, _, rot_1, inf = view_graph.focal_search_l1(gpu_ctx, n, i0, i1, R, 1000.0, [f])
        print(f"chain, focal {f}: rotations {np.abs(rot_1 - rot_t).max():.2e}, L1 cost {costs[t]:.2e}, get_cost {inf['get_costs'][0]:.6e} against {c[0]:.6e}")
        assert np.abs(rot_1 - rot_t).max() <= 1e-12
        assert abs(inf["get_costs"][0] - c[0]) <= 1e-12 * c[0]
    assert (costs <= 1e-9 * len(i0)).all() and (costs >= 0).all()


def _same(a, b, with_best=True):
    ok = np.array_equal(a[0], b[0]) and np.array_equal(a[3]["get_costs"], b[3]["get_costs"]) and np.array_equal(a[3]["iterations"], b[3]["iterations"])
    if with_best:
        ok = ok and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3]["residual"], b[3]["residual"]) and np.array_equal(a[3]["matches"], b[3]["matches"])
    return ok


def test_a_trial_does_not_depend_on_its_position(gpu_ctx, oracle, monkeypatch):
    n, i0, i1, R, _ = FR.f24(oracle)
    call = lambda f: view_graph.focal_search_l1(gpu_ctx, n, i0, i1, R, FR.FOCAL_GUESS, f, return_matches=True)
    a = call(FR.FOCALS)
    assert (a[3]["iterations"] >= 1).all() and len(set(a[0].tolist())) == 25
    assert _same(a, call(FR.FOCALS))                                                # the run
    r = call(FR.FOCALS[::-1])                                                       # the position
    assert np.array_equal(r[0][::-1], a[0]) and np.array_equal(r[3]["get_costs"][::-1], a[3]["get_costs"]) and np.array_equal(r[3]["iterations"][::-1], a[3]["iterations"])
    assert r[1] == 24 - a[1] and np.array_equal(r[2], a[2]) and np.array_equal(r[3]["residual"], a[3]["residual"]) and np.array_equal(r[3]["matches"], a[3]["matches"])
    pick = np.array([3, 24, 7, 0, 11, 19, 8])                                       # num_trials
    s = call(FR.FOCALS[pick])
    assert np.array_equal(s[0], a[0][pick]) and np.array_equal(s[3]["get_costs"], a[3]["get_costs"][pick]) and np.array_equal(s[3]["iterations"], a[3]["iterations"][pick])
    monkeypatch.setenv("SSFM_FOCAL_L1_SLAB_TRIALS", "4")                            # seven slabs, the last of one trial
    assert _same(a, call(FR.FOCALS))
    monkeypatch.delenv("SSFM_FOCAL_L1_SLAB_TRIALS")
    monkeypatch.setenv("SSFM_FOCAL_L1_FORCE_GLOBAL", "1")                           # the vectors and the records in global memory
    assert _same(a, call(FR.FOCALS))
    monkeypatch.setenv("SSFM_FOCAL_L1_SLAB_TRIALS", "4")
    assert _same(a, call(FR.FOCALS))


@pytest.mark.parametrize("seed", [1, 2])
def test_recovery_f60(gpu_ctx, oracle, seed):
    """The test that fails without the feature: the tree search is led astray by the corrupted tree edges, the L1 search is not."""
    n, i0, i1, R, bad = FR.f60(oracle, seed)
    ct, bt, _ = view_graph.focal_search_graph(gpu_ctx, n, i0, i1, R, FR.FOCAL_GUESS, FR.FOCALS)
    costs, best, rot, info = view_graph.focal_search_l1(gpu_ctx, n, i0, i1, R, FR.FOCAL_GUESS, FR.FOCALS)
    srt = np.sort(costs)
    print(f"F60({seed}): tree search {FR.FOCALS[bt]}, L1 search {FR.FOCALS[best]} (second / best cost {srt[1] / srt[0]:.4f}), iterations {info['iterations'].min()}-"
          f"{info['iterations'].max()}, kernel {info['kernel_ms']:.2f} ms for {len(FR.FOCALS)} trials")
    assert abs(FR.FOCALS[bt] - FR.FOCAL_TRUE) >= 250.0
    assert FR.FOCALS[best] == FR.FOCAL_TRUE


def test_recovery_f60_cut_at_the_found_focal(gpu_ctx, oracle):
    n, i0, i1, R, bad = FR.f60(oracle, 3)
    costs, best, rot, info = view_graph.focal_search_l1(gpu_ctx, n, i0, i1, R, FR.FOCAL_GUESS, FR.FOCALS, return_matches=True)
    assert FR.FOCALS[best] == FR.FOCAL_TRUE
    _, res, s = view_graph.initialize_rotations_l1(gpu_ctx, n, i0, i1, info["matches"])
    _, want_res, _ = FR.cut_at_best(oracle, 3)
    keep = res < FR.CUT
    print(f"F60(3): {s['iterations']} iterations at the found focal, kept {keep.sum()} of {len(keep)}, corrupted kept {(keep & bad).sum()}, clean dropped {(~keep & ~bad).sum()}")
    assert np.array_equal(keep, want_res < FR.CUT)
    assert not (keep & bad).any()


def test_refusals(gpu_ctx, oracle):
    n, i0, i1, R, _ = FR.f24(oracle)
    f = [900.0, 1000.0]
    bad0 = i0.copy(); bad0[5] = n
    for args, kw in (((n, i0, i1, R, 1300.0, f), dict(max_iterations=0)), ((n, i0, i1, R, 1300.0, f), dict(weight_floor=0.0)), ((n, i0, i1, R, 1300.0, f), dict(root=n)),
                     ((n, bad0, i1, R, 1300.0, f), {}), ((n, i0, i1, R, 1300.0, []), {})):
        with pytest.raises(_lib.SsfmError, match="ssfm error -1: ssfm_focal_search_l1"):
            view_graph.focal_search_l1(gpu_ctx, *args, **kw)
    costs, best, _, _ = view_graph.focal_search_l1(gpu_ctx, n, i0, i1, R, 1300.0, f)  # the context is fine afterwards
    assert np.isfinite(costs).all()
