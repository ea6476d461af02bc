#!/usr/bin/env python
"""Measure the robust rotation initialisation (ssfm_rot_l1_init, spherical_sfm_amd.view_graph.initialize_rotations_l1).

Graphs: all pairs of 200 / 500 / 2000 cameras with 30 % of the edges rotated by a further 20-170 degrees (the sizes of profiles/view_graph.json), and the shuffled
rings of tests/_rot_l1_ref.py (offsets 1, 2, 3, 5, 9, 15 % outliers) with 300 and 2000 cameras.  Per graph: --warmup calls, then --repeats timed calls of the whole
call (host tree + adjacency, uploads, every launch, downloads), the median is reported next to kernel_ms, the outer iteration count and the CG iteration count of
the last call, and the error of the start against the ground truth.  The same algorithm restated on the CPU of the same machine -- numpy for the residuals, a
scipy sparse direct solve (splu) for every weighted Laplacian -- is timed once per graph up to --cpu-max-edges edges (the Laplacian of an all-pairs graph is
dense; beyond that size the direct solve is left out and recorded as null).
"pipeline": what the start is for, on the rings of 60 cameras the tests use and on the ring of 300 -- the maximum error against the ground truth of the tree start, of
optimize_rotations from the tree start over all edges, of the L1 start, and of optimize_rotations from the L1 start over the edges the 2 degree cut keeps.
Writes profiles/rot_l1.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def all_pairs_graph(n, seed=0, outlier_frac=0.3, noise_deg=0.2):
    from spherical_sfm_amd import synth
    rng = np.random.default_rng(seed)
    R_gt = synth.so3exp(rng.normal(size=(n, 3)) * 0.8)
    a, b = np.triu_indices(n, 1)
    R = synth.so3exp(rng.normal(0.0, np.deg2rad(noise_deg), (len(a), 3))) @ R_gt[b] @ np.transpose(R_gt[a], (0, 2, 1))
    bad = rng.random(len(a)) < outlier_frac
    ax = rng.normal(size=(int(bad.sum()), 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    R[bad] = synth.so3exp(ax * np.deg2rad(rng.uniform(20.0, 170.0, (len(ax), 1)))) @ R[bad]
    return n, a.astype(np.int32), b.astype(np.int32), R, R_gt, bad


def cpu_sparse(n, i0, i1, rel, root=0, max_iterations=30, step_tolerance=1e-4, weight_floor=1e-3):
    """tests/_rot_l1_ref.l1_irls with scipy.sparse.linalg.splu in place of the dense solve (connected graphs without self loops) -> rotations, iterations"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    import _rot_l1_ref as RR
    from spherical_sfm_amd import synth, view_graph
    R = view_graph.initialize_rotations_tree(n, i0, i1, rel, root)
    free = np.ones(n, bool); free[root] = False
    idx = -np.ones(n, np.int64); idx[free] = np.arange(n - 1)
    ia, ib = idx[i0], idx[i1]; fa, fb = ia >= 0, ib >= 0; both = fa & fb
    for k in range(1, max_iterations + 1):
        v = RR.so3ln(np.transpose(R[i1], (0, 2, 1)) @ rel @ R[i0]); nv = np.linalg.norm(v, axis=1)
        w = 1.0 / np.maximum(nv, weight_floor)
        rows = np.concatenate([ia[fa], ib[fb], ia[both], ib[both]]); cols = np.concatenate([ia[fa], ib[fb], ib[both], ia[both]])
        vals = np.concatenate([w[fa], w[fb], -w[both], -w[both]])
        L = sp.coo_matrix((vals, (rows, cols)), shape=(n - 1, n - 1)).tocsc()
        g = np.zeros((n - 1, 3)); np.add.at(g, ib[fb], (w[:, None] * v)[fb]); np.add.at(g, ia[fa], -(w[:, None] * v)[fa])
        x = spl.splu(L).solve(g)
        R[free] = R[free] @ synth.so3exp(x)
        if np.linalg.norm(x, axis=1).max() < step_tolerance:
            break
    return R, k


def pipeline_rows(ctx):
    import _rot_l1_ref as RR
    from spherical_sfm_amd import rotavg, view_graph
    rows = []
    for n, seed in ((60, 0), (60, 4), (300, 0), (300, 1)):
        n, i0, i1, R, R_gt, bad = RR._ring(n, seed)
        err = lambda rot: RR.geodesic(rot @ rot[0].T, R_gt @ R_gt[0].T)                       # gauge: camera 0
        tree = view_graph.initialize_rotations_tree(n, i0, i1, R)
        tree_refined = rotavg.optimize_rotations(ctx, tree, i0, i1, R)[0]
        l1, res, s = view_graph.initialize_rotations_l1(ctx, n, i0, i1, R)
        keep = (res >= 0) & (res <= RR.CUT)
        connected = view_graph.spanning_tree(n, i0[keep], i1[keep], 0)["num_reached"] == n
        l1_refined = rotavg.optimize_rotations(ctx, l1, i0[keep], i1[keep], R[keep])[0]
        l1_refined_all = rotavg.optimize_rotations(ctx, l1, i0, i1, R)[0]
        row = dict(cameras=n, edges=int(len(i0)), seed=seed, tree_start_max_deg=float(np.rad2deg(err(tree).max())), tree_start_median_deg=float(np.rad2deg(np.median(err(tree)))),
                   tree_refined_all_edges_max_deg=float(np.rad2deg(err(tree_refined).max())), l1_start_max_deg=float(np.rad2deg(err(l1).max())),
                   l1_outer_iterations=s["iterations"], l1_termination=s["termination"], cut_2deg_outliers_kept=int((keep & bad).sum()),
                   cut_2deg_clean_dropped=int((~keep & ~bad).sum()), cut_graph_connected=bool(connected),
                   l1_refined_all_edges_max_deg=float(np.rad2deg(err(l1_refined_all).max())), l1_cut_refined_max_deg=float(np.rad2deg(err(l1_refined).max())))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all-pairs", type=int, nargs="*", default=[200, 500, 2000])
    ap.add_argument("--rings", type=int, nargs="*", default=[300, 2000])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-max-edges", type=int, default=200000)
    ap.add_argument("--pipeline-only", action="store_true", help="skip the timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rot_l1.json"))
    a = ap.parse_args()
    import _rot_l1_ref as RR
    from spherical_sfm_amd import ba, view_graph
    ctx = ba.Context(0)
    rows = []
    for kind, n in [] if a.pipeline_only else [("all_pairs", n) for n in a.all_pairs] + [("ring", n) for n in a.rings]:
        n, i0, i1, R, R_gt, bad = all_pairs_graph(n) if kind == "all_pairs" else RR._ring(n, 0)
        ms = []
        for it in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            rot, res, s = view_graph.initialize_rotations_l1(ctx, n, i0, i1, R)
            if it >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        err = RR.error_to_truth_deg(rot, R_gt, 0)
        tree = RR.error_to_truth_deg(view_graph.initialize_rotations_tree(n, i0, i1, R), R_gt, 0)
        keep = (res >= 0) & (res <= RR.CUT)
        row = dict(graph=kind, cameras=n, edges=int(len(i0)), outliers=int(bad.sum()), call_ms_median=float(np.median(ms)), call_ms_all=ms, kernel_ms=s["kernel_ms"],
                   outer_iterations=s["iterations"], termination=s["termination"], cg_iterations=s["pcg_iterations_total"], cg_solves_capped=s["pcg_solves_capped"],
                   cost_initial=s["initial_cost"], cost_final=s["final_cost"], tree_start_max_deg=float(tree.max()), tree_start_median_deg=float(np.median(tree)),
                   l1_start_max_deg=float(err.max()), l1_start_median_deg=float(np.median(err)), cut_2deg_outliers_kept=int((keep & bad).sum()),
                   cut_2deg_clean_dropped=int((~keep & ~bad).sum()), cpu_sparse_ms=None, cpu_sparse_iterations=None, cpu_sparse_max_diff_rad=None)
        if len(i0) <= a.cpu_max_edges:
            t0 = time.perf_counter()
            Rc, kc = cpu_sparse(n, i0, i1, R)
            row.update(cpu_sparse_ms=1e3 * (time.perf_counter() - t0), cpu_sparse_iterations=int(kc), cpu_sparse_max_diff_rad=float(RR.geodesic(rot, Rc).max()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = dict(warmup=a.warmup, repeats=a.repeats,
               what="whole call of initialize_rotations_l1 (host tree + adjacency, uploads, launches, downloads), defaults; cpu_sparse_ms: the numpy + scipy splu "
                    "restatement on the CPU of the same machine, once", graphs=rows, pipeline=pipeline_rows(ctx))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
