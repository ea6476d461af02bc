#!/usr/bin/env python
"""Measure the five-point LO-MSAC (ssfm_ransac5_batch) against the spherical three-point LO-MSAC (ssfm_ransac_batch) on the same pairs:
--pairs general-motion pairs of --corr correspondences (0.5 px noise at f = 1000, 30 % outliers), default options, min_num_inliers 20.

Writes profiles/r07_fivepoint.json: kernel ms (ssfm_ransac_last_kernel_ms) and call ms of both, per pair, and their ratio.  Warm-up calls first,
then --repeats timed calls; the median is reported.  The spherical estimator does not fit these pairs (that is what the five-point path is
for): the comparison prices the estimators' arithmetic -- up to ten candidates from a 10 x 20 elimination against four from a 3-point sample,
and five per iteration in num_required_iterations instead of three -- not their results."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--corr", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_fivepoint.json"))
    a = ap.parse_args()
    from spherical_sfm_amd import ba, ransac, synth
    probs = [synth.make_general_pose_problem(a.corr, noise_px=0.5, outlier_frac=0.3, focal=1000.0, seed=k) for k in range(a.pairs)]
    ptr = np.arange(a.pairs + 1, dtype=np.int32) * a.corr
    U = np.ascontiguousarray(np.concatenate([p[0] for p in probs])); V = np.ascontiguousarray(np.concatenate([p[1] for p in probs]))
    thr = (2.0 / 1000.0) ** 2
    ctx = ba.Context(0)
    rec = dict(pairs=a.pairs, correspondences=a.corr, warmup=a.warmup, repeats=a.repeats)
    for name, fn in (("five_point", lambda: ransac.ransac5_batch(ctx, ptr, U, V, thr, min_num_inliers=20)),
                     ("spherical", lambda: ransac.estimate_flat(ctx, ptr, U, V, thr, min_num_inliers=20))):
        kernel_ms, call_ms = [], []
        for it in range(a.warmup + a.repeats):
            t0 = time.perf_counter(); out = fn(); t1 = time.perf_counter()
            if it >= a.warmup:
                kernel_ms.append(ransac.last_kernel_ms(ctx)); call_ms.append(1e3 * (t1 - t0))
        k = float(np.median(kernel_ms))
        rec[name] = dict(kernel_ms_median=k, kernel_ms_all=kernel_ms, call_ms_median=float(np.median(call_ms)), kernel_us_per_pair=1e3 * k / a.pairs,
                         accepted=int((out["num_inliers"] > 20).sum()), mean_iterations=float(out["iterations"].mean()), mean_lo_runs=float(out["lo_runs"].mean()))
        if name == "five_point":
            err = [np.degrees(np.arccos(np.clip((np.trace(out["R"][i].T @ probs[i][2]) - 1) / 2, -1, 1))) for i in range(a.pairs)]
            rec[name]["median_rotation_error_deg"] = float(np.median(err))
    rec["kernel_time_ratio_five_point_over_spherical"] = rec["five_point"]["kernel_ms_median"] / rec["spherical"]["kernel_ms_median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    ctx.close()


if __name__ == "__main__":
    main()
