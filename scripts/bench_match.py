#!/usr/bin/env python
"""Measure the GPU descriptor matching (ssfm_match_pairs) on an exhaustive problem: 64 frames x 4000 integer descriptors = 2016 pairs.

Writes profiles/r07_match.json: kernel ms (ssfm_match_last_kernel_ms), call ms, pairs/s and the achieved FLOP/s of the distance product
(2 * 128 * sum n0 * n1 / kernel time) as a fraction of the f32 matrix peak of the MI355X (157.3 TF spec, 155 TF measured back to back).
Warm-up calls first, then --repeats timed calls; the median is reported.  Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_match.py`
the same run gives the per-kernel split."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--features", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_match.json"))
    a = ap.parse_args()
    import _match_ref as R
    from spherical_sfm_amd import ba, match
    pool = R.world_pool(2 * a.features, seed=1)
    frames = [R.integer_frame(pool, a.features, 100 + f)[0] for f in range(a.frames)]
    fp, d, _ = match._flatten(frames)
    pairs = np.array(match.exhaustive_pairs(a.frames), np.int32)
    ctx = ba.Context(0)
    n = np.diff(fp).astype(np.float64)
    flop = 2.0 * 128.0 * float((n[pairs[:, 0]] * n[pairs[:, 1]]).sum())
    kernel_ms, call_ms, total = [], [], 0
    for it in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        mp, m0, m1 = match.match_flat(ctx, fp, d, pairs[:, 0], pairs[:, 1])
        t1 = time.perf_counter()
        if it >= a.warmup:
            kernel_ms.append(match.last_kernel_ms(ctx)); call_ms.append(1e3 * (t1 - t0))
        total = int(mp[-1])
    # one pair against the restatement, so that the timed path is the checked path
    j, i = R.match_pair(frames[0], frames[1])
    assert np.array_equal(m0[mp[0]:mp[1]], j) and np.array_equal(m1[mp[0]:mp[1]], i)
    k = float(np.median(kernel_ms)); c = float(np.median(call_ms))
    rec = dict(frames=a.frames, features_per_frame=a.features, pairs=int(len(pairs)), matches=total, warmup=a.warmup, repeats=a.repeats,
               kernel_ms_median=k, kernel_ms_all=kernel_ms, call_ms_median=c, call_ms_all=call_ms, pairs_per_s_kernel=len(pairs) / (1e-3 * k),
               pairs_per_s_call=len(pairs) / (1e-3 * c), flop=flop, tflops_kernel=flop / (1e-3 * k) / 1e12,
               fraction_of_f32_matrix_peak_spec=flop / (1e-3 * k) / 157.3e12, fraction_of_f32_matrix_peak_measured=flop / (1e-3 * k) / 155e12)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    ctx.close()


if __name__ == "__main__":
    main()
