#!/usr/bin/env python
"""Times the stereo panorama stage (ssfm_pano_synthesize) at the size the reference is used at: 300 keyframes of 1920 x 1080 on a circle, pano_width 4096, nine
phis, flow mode.  The generator is seeded; frames and flows are made on the device with torch (smooth flows of a few pixels, random textures), every keyframe its
own, so nothing is served from a cache that a real sweep would miss.

Protocol: host-pointer calls (numpy in, staged in slabs, numpy out) and device-pointer calls (torch tensors in and out, nothing copied) alternate; medians of
--reps timed calls after --warmup untimed ones.  Per mode: the whole call (host clock round a call that ends in a stream synchronise: plan, uploads, kernels,
download) and the event-bracketed kernel time (ssfm_pano_last_kernel_ms).  The plan is timed on its own as well (host only).  Before any timing the two modes'
panoramas are compared byte for byte.

Byte model (algorithmic, per synthesised pixel): 3 output bytes + two frame samples of 3 bytes + two flow samples of 8 bytes = 25 bytes; the four taps of a
bilinear sample are neighbours and are counted once.  It is set against the copy bandwidth ssfm_debug_copy_bandwidth measures in the same run.

    python scripts/bench_pano.py [--out profiles/pano.json] [--notes profiles/pano_notes.md]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spherical_sfm_amd import _lib, ba, pano  # noqa: E402


def circle(n, rng):
    R, t = [], []
    for k in range(n):
        a = (k + rng.uniform(-0.3, 0.3)) * 2 * np.pi / n
        c, s = np.cos(a), np.sin(a)
        yaw = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
        rx, rz = rng.normal(0, 0.02, 2)
        tilt = np.array([[1, -rz, 0], [rz, 1, -rx], [0, rx, 1]]); u, _, vt = np.linalg.svd(tilt); tilt = u @ vt
        R.append(tilt @ yaw); t.append(np.array([0, 0, -1.0]) + rng.normal(0, 0.01, 3))
    return np.array(R), np.array(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=300); ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pano-width", type=int, default=4096); ap.add_argument("--num-phi", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pano.json")); ap.add_argument("--notes", default=os.path.join(ROOT, "profiles", "pano_notes.md"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_pano.py needs a GPU: there is no CPU path to time"
    dev = torch.device("cuda", 0)
    ctx = ba.Context(0)
    n, W, H, PW = a.keyframes, a.width, a.height, a.pano_width
    rng = np.random.default_rng(1)
    R, t = circle(n, rng)
    intr = (0.52 * W, W / 2 - 0.5, H / 2 - 0.5)
    g = torch.Generator(device=dev); g.manual_seed(2)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    frames_d, fwd_d, bwd_d = [], [], []
    for k in range(n):
        frames_d.append(torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g))
        for lst in (fwd_d, bwd_d):
            p = torch.rand(4, device=dev, generator=g)
            u = 3.0 * torch.sin(0.01 * (1 + p[0]) * xx + 6 * p[1]) * torch.cos(0.013 * (1 + p[2]) * yy + 6 * p[3])
            lst.append(torch.stack([u, -0.5 * u], dim=-1).contiguous())
    torch.cuda.synchronize(dev)
    frames_h = [f.cpu().numpy() for f in frames_d]; fwd_h = [f.cpu().numpy() for f in fwd_d]; bwd_h = [f.cpu().numpy() for f in bwd_d]
    opts = dict(num_phi=a.num_phi)

    t0 = time.perf_counter(); P = pano.plan(R, t, intr, W, H, PW, **opts); plan_s = time.perf_counter() - t0
    owned = int((P["owner"] >= 0).sum()); pixels = owned * H
    bw = C.c_double(0)
    _lib.check(_lib.lib().ssfm_debug_copy_bandwidth(ctx._p, 1 << 29, 5, C.byref(bw)), ctx._p)

    def host():
        t0 = time.perf_counter(); out = pano.synthesize(ctx, R, t, intr, frames_h, (fwd_h, bwd_h), pano_width=PW, **opts)
        return out, time.perf_counter() - t0, pano.last_kernel_ms(ctx)

    def device():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter(); out = pano.synthesize(ctx, R, t, intr, frames_d, (fwd_d, bwd_d), pano_width=PW, **opts); torch.cuda.synchronize(dev)
        return out, time.perf_counter() - t0, pano.last_kernel_ms(ctx)

    oh, _, _ = host(); od, _, _ = device()
    equal = bool(np.array_equal(oh, od.cpu().numpy()))
    assert equal, "host-pointer and device-pointer panoramas differ"
    for _ in range(max(a.warmup - 1, 0)):
        host(); device()
    rows = {"host": [], "device": []}
    for _ in range(a.reps):
        for name, fn in (("host", host), ("device", device)):
            _, call_s, k_ms = fn(); rows[name].append((call_s * 1e3, k_ms))
    model_bytes = pixels * 25
    upload_bytes = n * H * W * 3 + 2 * n * H * W * 8; download_bytes = a.num_phi * H * PW * 3
    res = {"scene": {"keyframes": n, "width": W, "height": H, "pano_width": PW, "num_phi": a.num_phi, "mode": "flow", "jobs": int(len(P["pair"])),
                     "columns_owned": owned, "columns": int(P["owner"].size), "pixels_synthesised": pixels},
           "protocol": {"reps": a.reps, "warmup": a.warmup, "alternating": True, "modes_equal_bytes": equal},
           "plan_ms_host_only": plan_s * 1e3, "copy_bandwidth_GBs": bw.value,
           "model_bytes": model_bytes, "model_bytes_per_pixel": 25, "model_ms_at_copy_bandwidth": model_bytes / (bw.value * 1e9) * 1e3,
           "host_mode_upload_bytes": upload_bytes, "host_mode_download_bytes": download_bytes}
    for name in rows:
        call = np.array([r[0] for r in rows[name]]); k = np.array([r[1] for r in rows[name]])
        res[name] = {"call_ms_median": float(np.median(call)), "call_ms_all": call.tolist(), "kernel_ms_median": float(np.median(k)), "kernel_ms_all": k.tolist(),
                     "kernel_model_GBs": model_bytes / (float(np.median(k)) * 1e-3) / 1e9, "kernel_share_of_copy_bandwidth": model_bytes / (float(np.median(k)) * 1e-3) / 1e9 / bw.value}
    res["host"]["upload_GBs_over_call"] = upload_bytes / (res["host"]["call_ms_median"] * 1e-3) / 1e9
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    kept = ""                                                            # the hand-written reading below the generated part survives a rerun
    if os.path.exists(a.notes):
        old = open(a.notes).read(); i = old.find("\n## Reading")
        kept = old[i:] if i >= 0 else ""
    with open(a.notes, "w") as f:
        s = res["scene"]
        f.write(f"""# Stereo panorama: first measurement (scripts/bench_pano.py)

Scene: {s['keyframes']} keyframes of {s['width']} x {s['height']}, pano_width {s['pano_width']}, {s['num_phi']} phis, flow mode; {s['jobs']} jobs, {s['columns_owned']} of {s['columns']} columns
owned, {s['pixels_synthesised']} pixels synthesised.  Host-pointer and device-pointer calls alternate, {a.reps} timed after {a.warmup} warm-up; their panoramas are equal byte for
byte ({equal}).

| | call ms (median) | kernel ms (median) | model GB/s over kernel time | share of copy bandwidth |
|---|---|---|---|---|
| device pointers | {res['device']['call_ms_median']:.1f} | {res['device']['kernel_ms_median']:.2f} | {res['device']['kernel_model_GBs']:.0f} | {res['device']['kernel_share_of_copy_bandwidth']:.3f} |
| host pointers | {res['host']['call_ms_median']:.1f} | {res['host']['kernel_ms_median']:.2f} | {res['host']['kernel_model_GBs']:.0f} | {res['host']['kernel_share_of_copy_bandwidth']:.3f} |

- Copy bandwidth measured in the same run (ssfm_debug_copy_bandwidth, 512 MiB): {bw.value:.0f} GB/s.  The byte model (25 bytes per pixel: 3 out, 2 x 3 frame, 2 x 8 flow)
  is {model_bytes / 1e9:.2f} GB, {res['model_ms_at_copy_bandwidth']:.2f} ms at that bandwidth.
- The plan alone (host, threads): {plan_s * 1e3:.0f} ms.  It is part of every call time above.
- Host-pointer mode moves {upload_bytes / 1e9:.2f} GB up and {download_bytes / 1e9:.2f} GB down per call: {res['host']['upload_GBs_over_call']:.1f} GB/s of upload over the whole call.
""")
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
