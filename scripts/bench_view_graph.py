#!/usr/bin/env python
"""Measure the triplet filter (ssfm_triplet_filter) and the spanning tree (ssfm_view_graph_tree) on all-pairs view graphs of 200, 500 and 2000 cameras
(the last is the graph of BASELINE configs[3]: 1 999 000 edges, 1.33e9 triplets).

Cameras on a one-axis ring with small per-edge noise, so both product orders see consistent triangles.  Per size: --warmup calls, then --repeats timed calls of
the whole C call (host CSR sort + uploads + kernel + download; no records), the median is reported; the tree is timed the same way on the host.  A 24-camera
sub-graph of the smallest graph is also checked against the numpy restatement of the reference loop, so that the timed path is the checked path.  Writes profiles/view_graph.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def all_pairs_graph(n, seed=0):
    from spherical_sfm_amd import synth
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n) / n
    R_gt = synth.so3exp(np.stack([np.zeros(n), np.where(ang > np.pi, ang - 2 * np.pi, ang), np.zeros(n)], axis=1))
    a, b = np.triu_indices(n, 1)
    noise = synth.so3exp(rng.normal(0.0, np.deg2rad(0.05), (len(a), 3)))
    return a.astype(np.int32), b.astype(np.int32), noise @ R_gt[b] @ np.transpose(R_gt[a], (0, 2, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 500, 2000])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_graph.json"))
    a = ap.parse_args()
    from spherical_sfm_amd import ba, view_graph
    ctx = ba.Context(0)
    thresh = np.deg2rad(2.0)
    rows = []
    for n in a.sizes:
        i0, i1, R = all_pairs_graph(n)
        row = dict(cameras=n, edges=int(len(i0)))
        for name, order in (("reference", view_graph.ORDER_REFERENCE), ("composed", view_graph.ORDER_COMPOSED)):
            ms = []
            for it in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                good, count = view_graph.triplet_filter(ctx, n, i0, i1, R, thresh, order)
                if it >= a.warmup:
                    ms.append(1e3 * (time.perf_counter() - t0))
            assert count == n * (n - 1) * (n - 2) // 6
            row.update({f"call_ms_median_{name}": float(np.median(ms)), f"call_ms_all_{name}": ms, f"good_edges_{name}": int(good.sum()), "triplets": int(count),
                        f"triplets_per_s_{name}": count / (1e-3 * float(np.median(ms)))})
        ms = []
        for it in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            tree = view_graph.spanning_tree(n, i0, i1, 0)
            if it >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        row.update(tree_ms_median=float(np.median(ms)), tree_levels=int(tree["num_levels"]), tree_reached=int(tree["num_reached"]))
        if n <= 200:                                                              # against the vectorised restatement of the reference's loops
            import _view_graph_ref as VR
            from oracle import oracle as O
            sub = (i0 < 24) & (i1 < 24)
            want = VR.triplet_filter(O, i0[sub], i1[sub], R[sub], thresh, VR.ORDER_REFERENCE)
            got = view_graph.triplet_filter(ctx, 24, i0[sub], i1[sub], R[sub], thresh, VR.ORDER_REFERENCE)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1]
            row["checked_against_reference_loop"] = True
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = dict(warmup=a.warmup, repeats=a.repeats, what="whole C call (host sort + uploads + kernel + download), no records", sizes=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
