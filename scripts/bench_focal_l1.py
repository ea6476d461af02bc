#!/usr/bin/env python
"""Measure the robust focal search (ssfm_focal_search_l1, spherical_sfm_amd.view_graph.focal_search_l1).

Graphs, both as the uncalibrated pipeline sees them (true focal 1000, rotations estimated at the guessed focal 1300, 0.05 degrees of noise) with 15 % of the edges
rotated by a further 20-170 degrees, cameras renumbered and the list shuffled: the ring of 300 cameras with offsets 1-5 (1500 edges, the recipe of
tests/_focal_l1_ref.py) and all pairs of 200 cameras (19900 edges).  1024 trial focals, drawn uniformly from [guess / 4, 2 guess] as the driver draws them.
Per graph, --warmup calls and then the median of --repeats timed calls of
  * focal_search_l1, the whole call (host tree + adjacency, uploads, launches, downloads) and its kernel_ms;
  * focal_search_graph on the same input: the price of robustness is the ratio of the two;
  * the composition the call replaces -- per trial focal_search_graph with one trial for the matches, then initialize_rotations_l1 on them with the search's
    options -- measured on the first --composition-trials trials and EXTRAPOLATED to 1024 (labelled so);
and the focal both searches pick against the truth (the nearest trial focal to 1000 is recorded beside them).
Writes profiles/focal_l1.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FOCAL_TRUE, FOCAL_GUESS = 1000.0, 1300.0


def all_pairs_uncalibrated(O, n, seed=0, outlier_frac=0.15, noise_deg=0.05):
    """all pairs a < b of a camera ring (rotations about y), estimated at the guessed focal like tests/_uncalib_graph.make_uncalibrated_loop, then corrupted,
    renumbered and shuffled like tests/_focal_l1_ref._corrupted_ring -> n, i0, i1, R, corrupted"""
    import _rot_l1_ref as RR
    from spherical_sfm_amd import synth
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n) / n
    R_gt = synth.so3exp(np.stack([np.zeros(n), np.where(ang > np.pi, ang - 2 * np.pi, ang), np.zeros(n)], axis=1))
    i0, i1 = np.triu_indices(n, 1)
    Tinv = np.diag([FOCAL_GUESS / FOCAL_TRUE, FOCAL_GUESS / FOCAL_TRUE, 1.0])
    R = np.zeros((len(i0), 3, 3))
    for k, (a, b) in enumerate(zip(i0, i1)):
        Rt = synth.so3exp(rng.normal(0.0, np.deg2rad(noise_deg), size=(1, 3)))[0] @ R_gt[b] @ R_gt[a].T
        r, _ = O.decompose_spherical_essential_matrix(Tinv @ O.make_spherical_essential_matrix(Rt, False) @ Tinv, False)
        R[k] = synth.so3exp(np.asarray(r)[None])[0]
    E = len(i0)
    bad = rng.choice(E, int(round(outlier_frac * E)), replace=False)
    for e in bad:
        R[e] = RR._axis_kick(rng, 20.0, 170.0) @ R[e]
    perm = rng.permutation(n); order = rng.permutation(E)
    mask = np.zeros(E, bool); mask[bad] = True
    return n, np.ascontiguousarray(perm[i0][order].astype(np.int32)), np.ascontiguousarray(perm[i1][order].astype(np.int32)), np.ascontiguousarray(R[order]), mask[order]


def timed(fn, warmup, repeats):
    ms = []
    for it in range(warmup + repeats):
        t0 = time.perf_counter()
        out = fn()
        if it >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=300)
    ap.add_argument("--all-pairs", type=int, default=200)
    ap.add_argument("--trials", type=int, default=1024)
    ap.add_argument("--composition-trials", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focal_l1.json"))
    a = ap.parse_args()
    import _focal_l1_ref as FR
    from oracle import oracle as O
    from spherical_sfm_amd import ba, view_graph
    O.lib()
    ctx = ba.Context(0)
    focals = np.random.default_rng(0).uniform(FOCAL_GUESS / 4, FOCAL_GUESS * 2, a.trials)
    rows = []
    for kind, fx in (("ring", FR._corrupted_ring(O, a.ring, 5, 0)), ("all_pairs", all_pairs_uncalibrated(O, a.all_pairs))):
        n, i0, i1, R, bad = fx
        (costs, best, rot, info), ms_l1 = timed(lambda: view_graph.focal_search_l1(ctx, n, i0, i1, R, FOCAL_GUESS, focals), a.warmup, a.repeats)
        (ct, bt, _), ms_tree = timed(lambda: view_graph.focal_search_graph(ctx, n, i0, i1, R, FOCAL_GUESS, focals), a.warmup, a.repeats)

        def composition():
            for f in focals[:a.composition_trials]:
                m = view_graph.focal_search_graph(ctx, n, i0, i1, R, FOCAL_GUESS, [f], return_matches=True)[3]
                view_graph.initialize_rotations_l1(ctx, n, i0, i1, m, **FR.DEFAULTS)
        _, ms_comp = timed(composition, a.warmup, a.repeats)
        comp_1024 = float(np.median(ms_comp)) * a.trials / a.composition_trials
        near = np.abs(focals - FOCAL_TRUE) <= 0.2 * FOCAL_TRUE
        row = dict(graph=kind, cameras=n, edges=int(len(i0)), outliers=int(bad.sum()), trials=a.trials, vectors_in_lds=bool((16 * n + 4 * len(i0)) * 8 + 512 <= 156 * 1024),
                   l1_call_ms_median=float(np.median(ms_l1)), l1_call_ms_all=ms_l1, l1_kernel_ms=info["kernel_ms"], outer_iterations_min=int(info["iterations"].min()),
                   outer_iterations_max=int(info["iterations"].max()), tree_call_ms_median=float(np.median(ms_tree)), tree_call_ms_all=ms_tree,
                   l1_over_tree=float(np.median(ms_l1) / np.median(ms_tree)), composition_trials_measured=a.composition_trials,
                   composition_ms_measured_median=float(np.median(ms_comp)), composition_ms_extrapolated_to_all_trials=comp_1024,
                   composition_extrapolated_over_l1=float(comp_1024 / np.median(ms_l1)), focal_true=FOCAL_TRUE,
                   nearest_trial_focal=float(focals[np.argmin(np.abs(focals - FOCAL_TRUE))]), l1_best_focal=float(focals[best]), tree_best_focal=float(focals[bt]),
                   l1_best_cost=float(costs[best]), l1_cost_at_nearest_trial=float(costs[np.argmin(np.abs(focals - FOCAL_TRUE))]),
                   l1_best_focal_within_20_percent_of_truth=float(focals[near][np.argmin(costs[near])]),
                   l1_second_best_over_best_cost=float(np.sort(costs)[1] / np.sort(costs)[0]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = dict(warmup=a.warmup, repeats=a.repeats,
               what="whole calls (host work, uploads, launches, downloads), defaults of ssfm_focal_search_l1 (10 outer iterations); composition_ms_extrapolated_to_all_trials "
                    "is EXTRAPOLATED from composition_trials_measured trials, not measured", graphs=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
