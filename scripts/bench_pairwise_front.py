#!/usr/bin/env python
"""Measure the pairwise front end (ssfm_pairwise_from_features) against the composition it is defined by -- match.match_flat, candidate selection in numpy,
ransac.estimate_indexed, mask unpacking: the host round trip of the lists and the mask through the Python wrappers.

Two sizes: --size ransac (16 384 pairs x ~500 matches: 128 frames of 500 features that all correspond, every frame paired with 128 partners) and
--size match (2016 pairs of 4000 x 4000 features: 64 frames, exhaustive -- the size of scripts/bench_match.py).  The two paths alternate, --repeats times each
after --warmup of each; wall time per call and the summed kernel time (ssfm_pairwise_front_last_kernel_ms; match + RANSAC brackets for the composition) are
reported with their spread, and the outputs of the two paths are compared.  Writes profiles/r08_pairwise_front_<size>.json.

--model fivepoint measures ssfm_pairwise5_from_features the same way: the composition is match.match_flat + ransac.ransac5_batch_indexed, the compared outputs
include t and E, and the record goes to profiles/pairwise5_front_<size>.json.  --partners shortens the pair list of --size ransac (the five-point kernel
costs more per pair than the spherical one).  No ratio is asserted: the comparator is the two-call composition."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scene(size, seed=1, partners=128):
    """-> feat_ptr, descs, rays, pairs.  Frame f sees the same world points from a camera on the unit sphere rotated by f * 0.5 degrees."""
    import _front_scene as S
    if size == "ransac":
        F, n = 128, 500
        frames = S.arc_frames((n,) * F, dim=128, seed=seed, step_deg=0.5, pool=n, wrong_frac=0.2, unrelated_frac=0.1)
        pairs = [(a, (a + 1 + k) % F) for a in range(F) for k in range(partners)]
        pairs = [(a, b) for a, b in pairs if a != b]
    else:
        F, n = 64, 4000
        frames = S.arc_frames((n,) * F, dim=128, seed=seed, step_deg=0.5, pool=2 * n, wrong_frac=0.1, unrelated_frac=0.1)
        pairs = [(a, b) for a in range(F) for b in range(a + 1, F)]
    fp, descs, rays = S.flatten(frames)
    return fp, descs, rays, np.asarray(pairs, np.int32), S.FOCAL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=("ransac", "match"), default="ransac")
    ap.add_argument("--model", choices=("spherical", "fivepoint"), default="spherical")
    ap.add_argument("--partners", type=int, default=128, help="--size ransac: partners per frame (1..128)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-inliers", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from spherical_sfm_amd import ba, match, pairwise, ransac
    fp, descs, rays, pairs, focal = scene(a.size, partners=max(1, min(a.partners, 128)))
    five = a.model == "fivepoint"
    thr = (2.0 / focal) ** 2
    ro = ransac.default_options(min_num_inliers=a.min_inliers)
    ctx = ba.Context(0)

    def front():
        t0 = time.perf_counter()
        r = (pairwise.pairwise5_from_features if five else pairwise.pairwise_from_features)(ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=thr)
        return 1e3 * (time.perf_counter() - t0), pairwise.last_kernel_ms(ctx), r

    def composed():
        t0 = time.perf_counter()
        mp, m0, m1 = match.match_flat(ctx, fp, descs, pairs[:, 0], pairs[:, 1])
        k = match.last_kernel_ms(ctx)
        cnt = np.diff(mp); cand = np.nonzero((cnt >= ro.min_num_inliers) & (cnt > 0))[0]
        sel = np.concatenate([np.arange(mp[p], mp[p + 1]) for p in cand]) if len(cand) else np.zeros(0, np.int64)
        cp = np.zeros(len(cand) + 1, np.int32); cp[1:] = np.cumsum(cnt[cand])
        c0 = m0[sel]; c1 = m1[sel]
        r = (ransac.ransac5_batch_indexed if five else ransac.estimate_indexed)(ctx, fp, rays, pairs[cand, 0], pairs[cand, 1], cp, c0, c1, thr, options=ro)
        k += ransac.last_kernel_ms(ctx)
        keep = r["mask"] != 0
        acc = np.nonzero(r["num_inliers"] > ro.min_num_inliers)[0]
        seg = np.repeat(np.arange(len(cand)), cnt[cand]); ok = keep & np.isin(seg, acc)
        out = dict(accepted_pair=cand[acc].astype(np.int32), R=r["R"][acc], inl_idx0=c0[ok], inl_idx1=c1[ok])
        if five:
            out.update(t=r["t"][acc], E=r["E"][acc])
        return 1e3 * (time.perf_counter() - t0), k, out

    rec = dict(model=a.model, size=a.size, partners=a.partners if a.size == "ransac" else None, pairs=int(len(pairs)), features=int(fp[-1]), warmup=a.warmup, repeats=a.repeats, min_num_inliers=a.min_inliers,
               front_call_ms=[], front_kernel_ms=[], composition_call_ms=[], composition_kernel_ms=[])
    for it in range(a.warmup + a.repeats):                      # alternating
        tf, kf, rf = front(); tc, kc, rc = composed()
        if it >= a.warmup:
            rec["front_call_ms"].append(tf); rec["front_kernel_ms"].append(kf); rec["composition_call_ms"].append(tc); rec["composition_kernel_ms"].append(kc)
    same = all(np.array_equal(getattr(rf, k), rc[k]) for k in ("accepted_pair", "R", "inl_idx0", "inl_idx1") + (("t", "E") if five else ()))
    rec.update(outputs_equal=bool(same), accepted=int(len(rf.accepted_pair)), matches=int(rf.match_count.sum()), inlier_matches=int(len(rf.inl_idx0)), calls_per_front=int(rf.calls),
               front_call_ms_median=float(np.median(rec["front_call_ms"])), front_kernel_ms_median=float(np.median(rec["front_kernel_ms"])),
               composition_call_ms_median=float(np.median(rec["composition_call_ms"])), composition_kernel_ms_median=float(np.median(rec["composition_kernel_ms"])))
    out = a.out or os.path.join(ROOT, "profiles", ("pairwise5_front_%s.json" if five else "r08_pairwise_front_%s.json") % a.size)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    ctx.close()


if __name__ == "__main__":
    main()
