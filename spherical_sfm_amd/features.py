"""Keypoint selection: adaptiveNonMaximalSuppresion of the reference (examples/spherical_sfm_tools.cpp:76-123) and the selection rule of
DetectorTracker::detect (:179-208) over ssfm_anms_batch -- every frame in one device call.  The detector and the descriptor are OpenCV's and stay outside:
anms() takes keypoints from any detector, select() hands what survives to the front end (match.match_flat, pairwise.pairwise_from_features)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_float_p, c_i32_p


def _flatten(keypoints_per_frame, responses_per_frame, num_to_keep):
    pts = [np.asarray(p, np.float32).reshape(-1, 2) for p in keypoints_per_frame]
    rs = [np.asarray(r, np.float32).reshape(-1) for r in responses_per_frame]
    if len(pts) != len(rs) or any(len(p) != len(r) for p, r in zip(pts, rs)):
        raise ValueError("keypoints and responses differ in length")
    F = len(pts)
    ptr = np.zeros(F + 1, np.int32); ptr[1:] = np.cumsum([len(p) for p in pts])
    xy = np.ascontiguousarray(np.concatenate(pts) if F else np.zeros((0, 2), np.float32), np.float32)
    resp = np.ascontiguousarray(np.concatenate(rs) if F else np.zeros(0, np.float32), np.float32)
    keep = np.ascontiguousarray(np.broadcast_to(np.asarray(num_to_keep, np.int64), (F,)) if np.ndim(num_to_keep) == 0 else np.asarray(num_to_keep, np.int64))
    if keep.shape != (F,):
        raise ValueError("num_to_keep: one value, or one per frame")
    if F and (keep.max() > 2**31 - 1 or keep.min() < -2**31):
        raise ValueError("num_to_keep out of range")
    return ptr, xy, resp, np.ascontiguousarray(keep, np.int32)


def _split(ptr, keep_ptr, keep_idx, radius):
    F = len(ptr) - 1
    lists = [keep_idx[keep_ptr[f]:keep_ptr[f + 1]].copy() for f in range(F)]
    if radius is None:
        return lists
    return lists, [radius[ptr[f]:ptr[f + 1]].copy() for f in range(F)]


def anms_flat(ctx, kp_ptr, xy, response, num_to_keep, force_j_chunks=0, return_radius=False):
    """The C call itself on the flat layout -> (keep_ptr [F+1], keep_idx [kept], radius [total] or None)."""
    ptr = np.ascontiguousarray(kp_ptr, np.int32); xy = np.ascontiguousarray(xy, np.float32); resp = np.ascontiguousarray(response, np.float32)
    keep = np.ascontiguousarray(num_to_keep, np.int32)
    if len(ptr) < 1 or len(keep) != len(ptr) - 1:
        raise ValueError("kp_ptr has one entry more than num_to_keep")
    F = len(ptr) - 1
    well_formed = ptr[0] == 0 and bool(np.all(np.diff(ptr) >= 0))           # anything else is the library's to refuse, before it reads xy or response
    total = int(ptr[-1]) if well_formed else 0
    if well_formed and (xy.size != 2 * total or resp.size != total):
        raise ValueError("xy and response do not have kp_ptr[-1] keypoints")
    o = _lib.AnmsOptionsC(); _lib.lib().ssfm_anms_default_options(o); o.force_j_chunks = int(force_j_chunks)
    kptr = np.zeros(F + 1, np.int32); kidx = np.zeros(max(total, 1), np.int32)
    rad = np.zeros(max(total, 1)) if return_radius else None
    p = ctx._p if ctx is not None else None
    _lib.check(_lib.lib().ssfm_anms_batch(p, F, ptr.ctypes.data_as(c_i32_p), xy.ctypes.data_as(c_float_p), resp.ctypes.data_as(c_float_p),
                                         keep.ctypes.data_as(c_i32_p), C.byref(o), kptr.ctypes.data_as(c_i32_p), kidx.ctypes.data_as(c_i32_p),
                                         rad.ctypes.data_as(c_double_p) if rad is not None else None), p)
    return kptr, kidx[:kptr[-1]], (rad[:total] if rad is not None else None)


def anms(ctx, keypoints_per_frame, responses_per_frame, num_to_keep=4000, return_radius=False, force_j_chunks=0):
    """keypoints_per_frame: per frame an (n, 2) array of pixel positions, responses_per_frame: its n detector responses (both taken as float32, what
    cv::KeyPoint holds); num_to_keep: one value or one per frame.  -> per frame the kept keypoints' indices into its input, strongest response first
    (equal responses by index); with return_radius also per frame the suppression radius of every INPUT keypoint (float64).
    A frame with fewer keypoints than num_to_keep comes back unchanged: indices 0 .. n-1, radii DBL_MAX."""
    ptr, xy, resp, keep = _flatten(keypoints_per_frame, responses_per_frame, num_to_keep)
    kptr, kidx, rad = anms_flat(ctx, ptr, xy, resp, keep, force_j_chunks, return_radius)
    return _split(ptr, kptr, kidx, rad)


def anms_host(keypoints_per_frame, responses_per_frame, num_to_keep=4000, return_radius=False, num_threads=1):
    """The same contract computed on the host by the library's plain implementation (ssfm_anms_batch_host): a cross-check and the CPU side of
    scripts/anms_timing.py.  anms() never falls back to it."""
    ptr, xy, resp, keep = _flatten(keypoints_per_frame, responses_per_frame, num_to_keep)
    F = len(ptr) - 1; total = int(ptr[-1])
    kptr = np.zeros(F + 1, np.int32); kidx = np.zeros(max(total, 1), np.int32); rad = np.zeros(max(total, 1)) if return_radius else None
    _lib.check(_lib.lib().ssfm_anms_batch_host(F, ptr.ctypes.data_as(c_i32_p), xy.ctypes.data_as(c_float_p), resp.ctypes.data_as(c_float_p),
                                              keep.ctypes.data_as(c_i32_p), int(num_threads), kptr.ctypes.data_as(c_i32_p), kidx.ctypes.data_as(c_i32_p),
                                              rad.ctypes.data_as(c_double_p) if rad is not None else None), None)
    return _split(ptr, kptr, kidx[:kptr[-1]], rad[:total] if rad is not None else None)


def last_kernel_ms(ctx):
    """device time of the kernels of the context's last anms() / select() call (ssfm_anms_last_kernel_ms)"""
    ms = C.c_double(0)
    _lib.check(_lib.lib().ssfm_anms_last_kernel_ms(ctx._p, C.byref(ms)), ctx._p)
    return ms.value


def select(ctx, points, responses, descs=None, existing=0, target=4000):
    """The selection rule of DetectorTracker::detect for every frame at once: ntokeep = max(0, target - existing) (existing: the features a frame already
    has, one value or one per frame); a frame with ntokeep == 0 is skipped and contributes nothing (:186-187); every other frame keeps what
    adaptiveNonMaximalSuppresion(keypoints, ntokeep) keeps, in its order.  points / responses as in anms(); descs: per frame (n, dim) or None.
    -> (feat_ptr [F+1] int32, descs (total, dim) float32 or None, xy (total, 2) float32, keep): the layout of match._flatten, feat_ptr and descs go straight
    into match.match_flat / pairwise.pairwise_from_features, xy becomes the rays once the intrinsics are applied; keep: per frame the kept indices."""
    F = len(points)
    ex = np.broadcast_to(np.asarray(existing, np.int64), (F,)) if np.ndim(existing) == 0 else np.asarray(existing, np.int64)
    if ex.shape != (F,):
        raise ValueError("existing: one value, or one per frame")
    ntokeep = np.maximum(0, int(target) - ex)
    live = [f for f in range(F) if ntokeep[f] > 0]
    keep = [np.zeros(0, np.int32) for _ in range(F)]
    if live:
        got = anms(ctx, [points[f] for f in live], [responses[f] for f in live], ntokeep[live])
        for f, k in zip(live, got):
            keep[f] = k
    pts = [np.asarray(p, np.float32).reshape(-1, 2) for p in points]
    ptr = np.zeros(F + 1, np.int32); ptr[1:] = np.cumsum([len(k) for k in keep])
    xy = np.ascontiguousarray(np.concatenate([p[k] for p, k in zip(pts, keep)]) if F else np.zeros((0, 2), np.float32), np.float32)
    d = None
    if descs is not None:
        ds = [np.asarray(x, np.float32) for x in descs]
        dims = {x.shape[1] for x in ds if x.ndim == 2 and x.shape[0] > 0}
        if len(dims) > 1:
            raise ValueError(f"frames with different descriptor lengths: {sorted(dims)}")
        dim = dims.pop() if dims else 128
        d = np.ascontiguousarray(np.concatenate([x.reshape(-1, dim)[k] for x, k in zip(ds, keep)]) if F else np.zeros((0, dim), np.float32), np.float32)
    return ptr, d, xy, keep
