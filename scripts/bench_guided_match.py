#!/usr/bin/env python
"""Measure guided matching (ssfm_guided_match_pairs) against the plain matcher (ssfm_match_pairs, the existing code and the baseline) on the SAME pairs:
the accepted pairs of the pairwise front end on a closed ring of 64 frames x 4000 features (integer descriptors, 0.3 px noise).

Writes profiles/guided_match.json: per call the device time of the kernels (ssfm_guided_match_last_kernel_ms / ssfm_match_last_kernel_ms, event brackets round
the distance kernel and the compaction) and the wall time of the call with its uploads and read-backs, the two calls ALTERNATING inside one process after
warm-up calls of both; medians, all samples, the ratio, the share of (query, train) entries the band admits on the first pair (from the probe's cand_count)
and the list lengths.  The first pair's guided list is held against the numpy restatement, so the timed path is the checked path.
Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_guided_match.py --out /dev/null` the same run gives the per-kernel split."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def ring(num, features, seed=3):
    """tests/_front_scene.ring_frames with features // 3 points per anchor camera, topped up with unrelated features to exactly `features` per frame"""
    import _front_scene as S
    per_cam = features // 3
    frames = S.ring_frames(num, per_cam, seed=seed, stray=False)
    rng = np.random.default_rng(seed + 1)
    out = []
    for xy, d in frames:
        k = features - len(xy)
        xy = np.concatenate([xy, rng.uniform([0, 0], [2 * S.CX, 2 * S.CY], (k, 2))]); d = np.concatenate([d, rng.integers(0, 256, (k, d.shape[1])).astype(np.float32)])
        out.append((xy, d))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--features", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--check", type=int, default=1, help="hold the first pair against the numpy restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_match.json"))
    a = ap.parse_args()
    import _front_scene as S
    import _guided_ref as G
    from spherical_sfm_amd import ba, match, pairwise, ransac
    frames = ring(a.frames, a.features)
    fp, descs, rays = S.flatten(frames)
    thr = (2.0 / S.FOCAL) ** 2
    ctx = ba.Context(0)
    pairs = np.array(match.exhaustive_pairs(a.frames), np.int32)
    t0 = time.perf_counter()
    res = pairwise.pairwise_from_features(ctx, descs, rays, fp, pairs, ransac_options=ransac.default_options(min_num_inliers=100), sq_thresh=thr)
    front_ms = 1e3 * (time.perf_counter() - t0)
    acc = pairs[res.accepted_pair]
    Es = pairwise.spherical_essential(res.R)
    f0 = np.ascontiguousarray(acc[:, 0]); f1 = np.ascontiguousarray(acc[:, 1])
    samples = dict(plain_kernel=[], plain_call=[], guided_kernel=[], guided_call=[])
    plain = guided = None
    for it in range(a.warmup + a.repeats):                                           # alternating: both see the same neighbours on a shared machine
        t0 = time.perf_counter(); plain = match.match_flat(ctx, fp, descs, f0, f1); t1 = time.perf_counter()
        pk = match.last_kernel_ms(ctx)
        t2 = time.perf_counter(); guided = match.guided_match_flat(ctx, fp, descs, rays, f0, f1, Es, thr); t3 = time.perf_counter()
        gk = match.guided_last_kernel_ms(ctx)
        if it >= a.warmup:
            samples["plain_kernel"].append(pk); samples["plain_call"].append(1e3 * (t1 - t0)); samples["guided_kernel"].append(gk); samples["guided_call"].append(1e3 * (t3 - t2))
    a0, b0 = int(acc[0, 0]), int(acc[0, 1])
    tr, u = descs[fp[a0]:fp[a0 + 1]], rays[fp[a0]:fp[a0 + 1]]; q, v = descs[fp[b0]:fp[b0 + 1]], rays[fp[b0]:fp[b0 + 1]]
    cnt = match.guided_knn_probe(ctx, tr, u, q, v, Es[0], thr)[2]
    checked = None
    if a.check:
        gap = G.band_gap(G.sampson(u, v, Es[0]), thr)
        if gap > 1e-9:
            j, i = G.guided_pair(tr, u, q, v, Es[0], thr)
            assert np.array_equal(guided[1][guided[0][0]:guided[0][1]], j) and np.array_equal(guided[2][guided[0][0]:guided[0][1]], i)
            assert np.array_equal(cnt, G.cand_mask(u, v, Es[0], thr).sum(1))
            checked = True
    med = {k: float(np.median(x)) for k, x in samples.items()}
    n = np.diff(fp).astype(np.float64)
    entries = float((n[f0] * n[f1]).sum())
    rec = dict(frames=a.frames, features_per_frame=a.features, pairs_exhaustive=int(len(pairs)), pairs_accepted=int(len(acc)), entries=entries,
               squared_threshold=thr, warmup=a.warmup, repeats=a.repeats, front_end_call_ms=front_ms,
               band_admits_first_pair=float(cnt.sum() / (n[a0] * n[b0])), first_pair_checked_against_restatement=checked,
               matches_front_end_inliers=int(res.inl_ptr[-1]), matches_plain=int(plain[0][-1]), matches_guided=int(guided[0][-1]),
               plain_kernel_ms_median=med["plain_kernel"], guided_kernel_ms_median=med["guided_kernel"], kernel_ratio_guided_over_plain=med["guided_kernel"] / med["plain_kernel"],
               plain_call_ms_median=med["plain_call"], guided_call_ms_median=med["guided_call"], call_ratio_guided_over_plain=med["guided_call"] / med["plain_call"],
               plain_tflops_kernel=2.0 * 128.0 * entries / (1e-3 * med["plain_kernel"]) / 1e12, guided_tflops_kernel=2.0 * 128.0 * entries / (1e-3 * med["guided_kernel"]) / 1e12,
               samples=samples)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k != "samples"}))
    ctx.close()


if __name__ == "__main__":
    main()
