"""Times ssfm_anms_batch on the GPU beside the library's host implementation (ssfm_anms_batch_host) on the same input, and checks that the two return the same
keep lists and the same radius bits.  The figures of profiles/anms_notes.md come from this script.
usage: python scripts/anms_timing.py [--frames 300] [--n 20000] [--keep 4000] [--threads 16] [--reps 5] [--host-reps 2] [--json out.json]
Two shapes: `frames` frames of n keypoints (no j split: the frames fill the device) and one frame of n (the j-split case).  Device time is
ssfm_anms_last_kernel_ms (one event pair round the launches of a call); the call time is a host clock round the whole call, copies included.  Every shape is
warmed up twice before it is timed.  A pair evaluation is one (i, j) of a frame: n^2 per frame on the device, which compares every keypoint with every other;
the host walks only the prefix of stronger keypoints, so its pair count is lower and only its time is reported.  FP64 work per evaluation: one multiply and one
fused multiply-add (3 flop); the peak it is set against is the FP64 vector rate of the MI355X data sheet, 78.6 Tflop/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_VECTOR_PEAK = 78.6e12


def make(frames, n, seed):
    rng = np.random.default_rng(seed)
    pts = [np.stack([rng.uniform(0, 1920, n), rng.uniform(0, 1080, n)], axis=1).astype(np.float32) for _ in range(frames)]
    resp = [(rng.uniform(0, 1, n) ** 3 * 0.1).astype(np.float32) for _ in range(frames)]
    return pts, resp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300); ap.add_argument("--n", type=int, default=20000); ap.add_argument("--keep", type=int, default=4000)
    ap.add_argument("--threads", type=int, default=16); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("anms_timing.py needs a GPU: there is nothing to time without one")
    from spherical_sfm_amd import ba, features
    ctx = ba.Context(0)
    out = {"n": a.n, "keep": a.keep, "threads": a.threads, "shapes": []}
    for frames, reps in ((a.frames, a.reps), (1, 4 * a.reps)):
        pts, resp = make(frames, a.n, 1)
        ptr, xy, r, keep = features._flatten(pts, resp, a.keep)
        for _ in range(2):
            features.anms_flat(ctx, ptr, xy, r, keep)
        dev_ms, call_ms = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            kptr, kidx, rad = features.anms_flat(ctx, ptr, xy, r, keep, return_radius=True)
            call_ms.append(1e3 * (time.perf_counter() - t0)); dev_ms.append(features.last_kernel_ms(ctx))
        host_ms = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            hk, hr = features.anms_host(pts, resp, a.keep, return_radius=True, num_threads=a.threads)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        same = all(np.array_equal(kidx[kptr[f]:kptr[f + 1]], hk[f]) and np.array_equal(rad[ptr[f]:ptr[f + 1]].view(np.uint64), hr[f].view(np.uint64)) for f in range(frames))
        pairs = float(frames) * a.n * a.n
        best = min(dev_ms)
        row = {"frames": frames, "device_kernel_ms": dev_ms, "device_call_ms": call_ms, "host_ms": host_ms, "device_equals_host": bool(same),
               "kept_per_frame_mean": float(np.diff(kptr).mean()), "pair_evaluations": pairs, "pair_evaluations_per_s": pairs / (best * 1e-3),
               "fp64_flop_per_s": 3.0 * pairs / (best * 1e-3), "fraction_of_fp64_vector_peak": 3.0 * pairs / (best * 1e-3) / FP64_VECTOR_PEAK,
               "host_over_device_kernel": min(host_ms) / best}
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
        assert same, "the device and the host implementation disagree"
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
