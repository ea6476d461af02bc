"""Stereo panorama synthesis: make_stereo_panoramas of the reference (examples/stereo_panorama_tools.cpp:404-637) from levelled poses, frames and optional
optical flow, over ssfm_pano_plan / ssfm_pano_synthesize.  The flow estimator stays outside, like SIFT: flows are an input, and without them the call computes
the reference's synthesize_column_linear.  numpy arrays go through the host-pointer mode (staged in slabs), torch CUDA tensors through the device-pointer mode
(no copies, the result is a torch tensor on the same device)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_i32_p, c_u8_p

OPTION_NAMES = ("num_phi", "is_loop", "phi_step_deg", "depth", "synth_radius", "synth_focal_factor", "subpixel_bits", "on_device", "max_slab_bytes")


def options(**kw):
    """ssfm_pano_options with the reference's values (9 phis one degree apart, depth 10, radius 0.5, focal factor 1.2, a closed loop), then **kw."""
    o = _lib.PanoOptionsC(); _lib.lib().ssfm_pano_default_options(o)
    for k, v in kw.items():
        if k not in OPTION_NAMES:
            raise TypeError(f"unknown panorama option {k!r}")
        setattr(o, k, type(getattr(o, k))(v))
    return o


def _poses(R, t):
    R = np.ascontiguousarray(R, np.float64).reshape(-1, 3, 3); t = np.ascontiguousarray(t, np.float64).reshape(-1, 3)
    if len(R) != len(t):
        raise ValueError("R and t differ in length")
    return R, t


def plan(R, t, intrinsics, width, height, pano_width, **opts):
    """The column jobs and the owner map (host only, no GPU).  R (n, 3, 3) row-major, x_cam = R x_world + t; intrinsics = (focal, cx, cy).
    -> dict: pair, theta, phi, col (int32), ok (uint8), alpha, tan_phi (float64), synth_R (jobs, 3, 3), owner (num_phi, pano_width) int32 with -1 = none."""
    R, t = _poses(R, t); n = len(R); o = options(**opts); L = _lib.lib()
    focal, cx, cy = (float(v) for v in intrinsics)
    owner = np.full((max(int(o.num_phi), 0), max(int(pano_width), 0)), -1, np.int32)
    count = C.c_int32(0)
    args = (C.byref(o), n, R.ctypes.data_as(c_double_p), t.ctypes.data_as(c_double_p), focal, cx, cy, int(width), int(height), int(pano_width))
    rc = L.ssfm_pano_plan(*args, C.byref(count), None, None, None, None, None, None, None, owner.ctypes.data_as(c_i32_p))
    if rc != 0 and count.value <= 0:
        _lib.check(rc, None)
    m = count.value; cap = max(m, 1)
    ji = [np.zeros(cap, np.int32) for _ in range(4)]; ok = np.zeros(cap, np.uint8); alpha = np.zeros(cap); consts = np.zeros((cap, 10))
    count = C.c_int32(m)
    _lib.check(L.ssfm_pano_plan(*args, C.byref(count), *(a.ctypes.data_as(c_i32_p) for a in ji), ok.ctypes.data_as(c_u8_p), alpha.ctypes.data_as(c_double_p),
                                consts.ctypes.data_as(c_double_p), owner.ctypes.data_as(c_i32_p)), None)
    return {"pair": ji[0][:m], "theta": ji[1][:m], "phi": ji[2][:m], "col": ji[3][:m], "ok": ok[:m], "alpha": alpha[:m], "tan_phi": consts[:m, 0].copy(),
            "synth_R": consts[:m, 1:].reshape(m, 3, 3).copy(), "owner": owner}


def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _pointer_table(items, n, dtype, shape, what, device):
    """n pointers to C-contiguous arrays of `shape`; returns (table, keep-alive list)"""
    if len(items) != n:
        raise ValueError(f"{what}: {len(items)} entries for {n} keyframes")
    keep, tab = [], (C.c_void_p * max(n, 1))()
    for i, a in enumerate(items):
        if a is None:
            tab[i] = None
            continue
        if device:
            if not (_is_torch(a) and a.is_cuda):
                raise ValueError(f"{what}: torch CUDA tensors and numpy arrays cannot be mixed")
            if a.dtype != dtype[1] or tuple(a.shape) != shape:
                raise ValueError(f"{what}[{i}]: expected {dtype[1]} of shape {shape}")
            a = a.contiguous(); tab[i] = a.data_ptr()
        else:
            a = np.ascontiguousarray(a, dtype[0])
            if a.shape != shape:
                raise ValueError(f"{what}[{i}]: expected shape {shape}, got {a.shape}")
            tab[i] = a.ctypes.data
        keep.append(a)
    return tab, keep


def synthesize(ctx, R, t, intrinsics, frames, flows=None, pano_width=4096, return_owner=False, **opts):
    """frames: n images (height, width, 3) uint8, channel order kept; flows: None (linear mode) or (forward, backward), each n fields (height, width, 2) float32
    with entry k the flow of frame k -> k+1 (mod n) resp. of frame k+1 -> k (the entry of a pair that does not exist may be None).
    numpy in -> numpy out (num_phi, height, pano_width, 3) uint8; torch CUDA tensors in -> a torch tensor on their device, nothing copied.
    return_owner: also the owner map (num_phi, pano_width) int32, the pair each column was synthesised from, -1 = none (the column is black)."""
    R, t = _poses(R, t); n = len(R); L = _lib.lib()
    focal, cx, cy = (float(v) for v in intrinsics)
    frames = list(frames)
    device = any(_is_torch(f) for f in frames)
    if n == 0 or len(frames) == 0:
        raise ValueError("no keyframes")
    height, width = int(frames[0].shape[0]), int(frames[0].shape[1])
    o = options(**opts); o.on_device = 1 if device else 0
    torch = None
    if device:
        import torch
    ftab, keep = _pointer_table(frames, n, (np.uint8, torch.uint8 if device else None), (height, width, 3), "frames", device)
    fftab = fbtab = None
    if flows is not None:
        fwd, bwd = flows
        fftab, k1 = _pointer_table(list(fwd), n, (np.float32, torch.float32 if device else None), (height, width, 2), "flows[0]", device)
        fbtab, k2 = _pointer_table(list(bwd), n, (np.float32, torch.float32 if device else None), (height, width, 2), "flows[1]", device)
        keep += k1 + k2
    shape = (max(int(o.num_phi), 0), height, max(int(pano_width), 0), 3)
    owner = np.full((shape[0], shape[2]), -1, np.int32)
    if device:
        dev = keep[0].device
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)                                  # the inputs were produced on torch's streams; the library works on the context's
        optr = C.c_void_p(out.data_ptr())
    else:
        out = np.empty(shape, np.uint8)
        optr = C.c_void_p(out.ctypes.data)
    p = ctx._p if ctx is not None else None
    _lib.check(L.ssfm_pano_synthesize(p, C.byref(o), n, R.ctypes.data_as(c_double_p), t.ctypes.data_as(c_double_p), focal, cx, cy, width, height,
                                      ftab, fftab, fbtab, int(pano_width), optr, owner.ctypes.data_as(c_i32_p)), p)
    return (out, owner) if return_owner else out


def last_kernel_ms(ctx):
    """device time of the kernels of the context's last synthesize() call (ssfm_pano_last_kernel_ms)"""
    ms = C.c_double(0)
    _lib.check(_lib.lib().ssfm_pano_last_kernel_ms(ctx._p, C.byref(ms)), ctx._p)
    return ms.value
