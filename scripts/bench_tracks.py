#!/usr/bin/env python
"""Times build_sfm's track pass on the host (ssfm_build_tracks, merge = 1: one CPU thread) against the device call (ssfm_build_tracks_device) on a ring:
300 frames x 4000 features, every frame matched to its 10 successors, at wrong-match rates 0, 0.1 % and 1 %.  The generator is seeded.

Scene: world points on a circle; frame k sees the points k * stride .. k * stride + features - 1 (modulo the circle) as its features 0 .. features - 1, so
the match set (k, k + d) pairs feature j with feature j - d * stride.  A wrong match re-points the second feature at a random feature of its frame.

Protocol: the two calls alternate; medians of --reps timed runs after --warmup untimed ones.  A host call that takes longer than --slow-s seconds is timed
--slow-reps times after a single warm-up instead (the row says how often it ran), so that the 1 % row stays affordable.  The device figure is the whole call
(staging, transfers, kernels, the host pass over the observations) and, separately, the event-bracketed kernel time.  A host call in between leaves the device
call a cold host (caches, freed heap): the same number of device calls is then timed back to back as well, and the row holds both.  Before any timing the two outputs are
checked under the relation of include/ssfm.h: same partition, alive ids = components, same observation keys, equal pixels on single-feature keys.

    python scripts/bench_tracks.py [--out profiles/tracks_device.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spherical_sfm_amd import _lib, ba, tracks  # noqa: E402
from spherical_sfm_amd._lib import c_double_p, c_i32_p, c_i64_p, c_u8_p  # noqa: E402


def ring(frames, features, successors, stride, rate, seed):
    rng = np.random.default_rng(seed)
    fptr = (np.arange(frames + 1, dtype=np.int64) * features).astype(np.int32)
    fxy = rng.uniform(0.0, 2000.0, (frames * features, 2))
    i0, i1, f0, f1, mptr = [], [], [], [], [0]
    for k in range(frames):
        for d in range(1, successors + 1):
            a = np.arange(min(d * stride, features), features, dtype=np.int32)
            b = a - d * stride
            wrong = rng.random(len(a)) < rate
            b = np.where(wrong, rng.integers(0, features, len(a)), b).astype(np.int32)
            i0.append(k); i1.append((k + d) % frames); f0.append(a); f1.append(b); mptr.append(mptr[-1] + len(a))
    return (fptr, fxy, np.array(i0, np.int32), np.array(i1, np.int32), np.array(mptr, np.int32), np.concatenate(f0), np.concatenate(f1))


class Host:
    """ssfm_build_tracks on the flat arrays, output buffers allocated once"""

    def __init__(self, flat):
        self.flat = flat
        n = max(1, len(flat[5]))
        self.tracks = np.zeros(int(flat[0][-1]), np.int32); self.alive = np.zeros(n, np.uint8)
        self.oc = np.zeros(2 * n, np.int32); self.op = np.zeros(2 * n, np.int32); self.oxy = np.zeros((2 * n, 2))
        self.npts = C.c_int32(0); self.nobs = C.c_int64(0)

    def __call__(self, cx, cy):
        fptr, fxy, i0, i1, mptr, f0, f1 = self.flat
        p = lambda a, t: a.ctypes.data_as(t)
        rc = _lib.lib().ssfm_build_tracks(len(fptr) - 1, p(fptr, c_i32_p), p(fxy, c_double_p), len(i0), p(i0, c_i32_p), p(i1, c_i32_p), p(mptr, c_i32_p), p(f0, c_i32_p),
                                          p(f1, c_i32_p), cx, cy, 1, p(self.tracks, c_i32_p), C.byref(self.npts), p(self.alive, c_u8_p), C.byref(self.nobs),
                                          p(self.oc, c_i32_p), p(self.op, c_i32_p), p(self.oxy, c_double_p))
        assert rc == 0, rc
        n = self.nobs.value
        return dict(tracks=self.tracks, num_points=self.npts.value, alive=self.alive[:self.npts.value], obs_cam=self.oc[:n], obs_pt=self.op[:n], obs_xy=self.oxy[:n])


def check_relation(host, dev, fptr):
    """same partition, alive ids = components, same keys, equal pixels on single-feature keys (vectorised) -> (keys, single-feature keys)"""
    t = host["tracks"]; named = t >= 0
    ids, first = np.unique(t[named], return_index=True)                      # first = position among the named features: ascends with the global id
    rank = np.empty(len(ids), np.int64); rank[np.argsort(first, kind="stable")] = np.arange(len(ids))
    lut = np.full(int(host["num_points"]) + 1, -1, np.int64); lut[ids] = rank
    canon = np.where(named, lut[np.maximum(t, 0)], -1)
    assert np.array_equal(canon, dev["tracks"]), "partitions differ"
    assert int(np.count_nonzero(host["alive"])) == dev["num_points"] == len(ids), "alive ids != components"
    hk = host["obs_cam"].astype(np.int64) << 32 | lut[host["obs_pt"]]
    dk = dev["obs_cam"].astype(np.int64) << 32 | dev["obs_pt"].astype(np.int64)
    ho, do = np.argsort(hk), np.argsort(dk)
    assert np.array_equal(hk[ho], dk[do]) and (np.diff(dk[do]) > 0).all(), "observation keys differ"
    cam_of = np.searchsorted(fptr.astype(np.int64), np.arange(len(t)), side="right") - 1
    mk, cnt = np.unique(cam_of[named] << 32 | canon[named], return_counts=True)
    assert np.array_equal(mk, dk[do])
    single = cnt == 1
    assert np.array_equal(host["obs_xy"][ho][single], dev["obs_xy"][do][single]), "pixels differ on single-feature keys"
    return len(mk), int(single.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300); ap.add_argument("--features", type=int, default=4000); ap.add_argument("--successors", type=int, default=10)
    ap.add_argument("--stride", type=int, default=411); ap.add_argument("--rates", type=float, nargs="+", default=[0.0, 0.001, 0.01])
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--slow-s", type=float, default=20.0); ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_device.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    ctx = ba.Context(0)
    cx, cy = 960.0, 540.0
    rows = []
    for rate in a.rates:
        flat = ring(a.frames, a.features, a.successors, a.stride, rate, a.seed)
        host = Host(flat)
        dev_call = lambda: tracks.build_tracks_device_flat(ctx, *flat, cx, cy)
        t0 = time.perf_counter(); h = host(cx, cy); first_host_s = time.perf_counter() - t0
        d = dev_call()
        keys, single = check_relation(h, d, flat[0])
        slow = first_host_s > a.slow_s
        # True = timed.  The checked call above is a slow host's single warm-up
        host_plan = [True] * a.slow_reps if slow else [False] * a.warmup + [True] * a.reps
        dev_plan = [False] * a.warmup + [True] * a.reps
        host_warm = 1 if slow else a.warmup
        host_ms, call_ms, kern_ms = [], [], []
        for i in range(max(len(host_plan), len(dev_plan))):                               # alternating
            if i < len(host_plan):
                t0 = time.perf_counter(); host(cx, cy); dt = 1e3 * (time.perf_counter() - t0)
                if host_plan[i]: host_ms.append(dt)
                print(f"rate {rate}: host run {i} {dt:.1f} ms", file=sys.stderr, flush=True)
            if i < len(dev_plan):
                t0 = time.perf_counter(); dev_call(); dt = 1e3 * (time.perf_counter() - t0)
                if dev_plan[i]: call_ms.append(dt); kern_ms.append(tracks.last_kernel_ms(ctx))
        alone_ms = []                                                                     # the device call back to back, no host call in between
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter(); dev_call(); dt = 1e3 * (time.perf_counter() - t0)
            if i >= a.warmup: alone_ms.append(dt)
        row = dict(wrong_match_rate=rate, matches=int(len(flat[5])), match_sets=int(len(flat[2])), features=int(flat[0][-1]), points=int(d["num_points"]),
                   observations=int(d["num_observations"]), conflicted_points=int(d["conflict"].sum()), host_ids_issued=int(h["num_points"]),
                   observation_keys=keys, single_feature_keys=single, outputs_checked_equal=True,
                   host_ms_median=float(np.median(host_ms)), host_ms=host_ms, host_runs_timed=len(host_ms), host_warmups=host_warm,
                   device_call_ms_median=float(np.median(call_ms)), device_call_ms=call_ms, device_kernel_ms_median=float(np.median(kern_ms)), device_kernel_ms=kern_ms,
                   device_call_back_to_back_ms_median=float(np.median(alone_ms)), device_call_back_to_back_ms=alone_ms,
                   device_runs_timed=len(call_ms), device_warmups=a.warmup)
        row["host_over_device_call"] = row["host_ms_median"] / row["device_call_ms_median"]
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not isinstance(v, list)}), flush=True)
    out = dict(what="ssfm_build_tracks (host, merge = 1, one CPU thread) against ssfm_build_tracks_device (whole call and event-bracketed kernels), scripts/bench_tracks.py",
               device=torch.cuda.get_device_name(0), frames=a.frames, features_per_frame=a.features, successors=a.successors, stride=a.stride, seed=a.seed,
               protocol=f"alternating runs, medians of {a.reps} after {a.warmup} warm-ups; a host call slower than {a.slow_s} s: {a.slow_reps} timed runs after 1 warm-up",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
