"""Python host side of the track assignment of build_sfm (examples/spherical_sfm_tools.cpp:862-950): ssfm_build_tracks, the host bookkeeping, and
ssfm_build_tracks_device, the same tracks as connected components with canonical ids on the device (include/ssfm.h)."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import c_double_p, c_i32_p, c_u8_p, c_i64_p


def _flatten(features, image_matches):
    """-> (fptr [K+1], fxy [total, 2], i0 [S], i1 [S], mptr [S+1], f0 [M], f1 [M]); a match list as std::map<size_t,size_t> holds it: unique first index, ascending"""
    K = len(features)
    fptr = np.zeros(K + 1, np.int32)
    for k, f in enumerate(features):
        fptr[k + 1] = fptr[k] + len(f)
    fxy = np.ascontiguousarray(np.concatenate([np.asarray(f, np.float64).reshape(-1, 2) for f in features])) if fptr[-1] else np.zeros((0, 2))
    S = len(image_matches)
    i0 = np.array([m[0] for m in image_matches], np.int32); i1 = np.array([m[1] for m in image_matches], np.int32)
    mptr = np.zeros(S + 1, np.int32); f0, f1 = [], []
    for s, m in enumerate(image_matches):
        pairs = sorted(dict(m[2]).items())            # std::map<size_t,size_t>: unique first index, ascending
        mptr[s + 1] = mptr[s] + len(pairs); f0 += [a for a, _ in pairs]; f1 += [b for _, b in pairs]
    return fptr, fxy, i0, i1, mptr, np.array(f0, np.int32), np.array(f1, np.int32)


def build_tracks(features, image_matches, centerx=0.0, centery=0.0, merge=True):
    """features: list (per keyframe) of (n_k,2) pixel arrays.  image_matches: list of (index0, index1, [(f0,f1),...]).
    -> dict(tracks [list of int arrays per keyframe], num_points, alive (bool), obs_cam, obs_pt, obs_xy)."""
    K = len(features)
    fptr, fxy, i0, i1, mptr, f0, f1 = _flatten(features, image_matches)
    S = len(image_matches)
    npairs = max(1, len(f0))
    tracks = np.zeros(int(fptr[-1]), np.int32); npts = C.c_int32(0); alive = np.zeros(npairs, np.uint8); nobs = C.c_int64(0)
    oc = np.zeros(2 * npairs, np.int32); op = np.zeros(2 * npairs, np.int32); oxy = np.zeros((2 * npairs, 2))
    p = lambda a, t: a.ctypes.data_as(t)
    rc = _lib.lib().ssfm_build_tracks(K, p(fptr, c_i32_p), p(fxy, c_double_p), S, p(i0, c_i32_p), p(i1, c_i32_p), p(mptr, c_i32_p), p(f0, c_i32_p),
                                      p(f1, c_i32_p), centerx, centery, 1 if merge else 0, p(tracks, c_i32_p), C.byref(npts), p(alive, c_u8_p),
                                      C.byref(nobs), p(oc, c_i32_p), p(op, c_i32_p), p(oxy, c_double_p))
    if rc != 0:
        raise _lib.SsfmError(f"ssfm_build_tracks failed ({rc})")
    n = nobs.value
    return dict(tracks=[tracks[fptr[k]:fptr[k + 1]].copy() for k in range(K)], num_points=npts.value, alive=alive[:npts.value].astype(bool),
                obs_cam=oc[:n].copy(), obs_pt=op[:n].copy(), obs_xy=oxy[:n].copy())


def build_tracks_device_flat(ctx, feat_ptr, feat_xy, ms_index0, ms_index1, ms_ptr, m_f0, m_f1, centerx=0.0, centery=0.0, observations=True):
    """The C call itself on the flat arrays of include/ssfm.h (nothing is sorted or made unique: the call does not need it).
    -> dict(tracks [total] int32, num_points, conflict [num_points] bool, obs_cam, obs_pt, obs_feat, obs_xy [n, 2]); observations=False only counts:
    the four lists are None and num_observations holds the count."""
    fptr = np.ascontiguousarray(feat_ptr, np.int32); fxy = np.ascontiguousarray(feat_xy, np.float64)
    i0 = np.ascontiguousarray(ms_index0, np.int32); i1 = np.ascontiguousarray(ms_index1, np.int32); mptr = np.ascontiguousarray(ms_ptr, np.int32)
    f0 = np.ascontiguousarray(m_f0, np.int32); f1 = np.ascontiguousarray(m_f1, np.int32)
    if len(i0) != len(i1) or len(mptr) != len(i0) + 1 or len(f0) != len(f1):
        raise ValueError("ms_index0 / ms_index1 / ms_ptr or m_f0 / m_f1 differ in length")
    K = len(fptr) - 1
    total = max(int(fptr[-1]), 0) if K >= 0 and len(fptr) else 0
    cap = max(total, 1)
    tracks = np.empty(cap, np.int32); conflict = np.zeros(cap, np.uint8); npts = C.c_int32(0); nobs = C.c_int64(0)
    p = lambda a, t: a.ctypes.data_as(t)
    if observations:
        oc = np.empty(cap, np.int32); op = np.empty(cap, np.int32); of = np.empty(cap, np.int32); oxy = np.empty((cap, 2))
        outs = (p(oc, c_i32_p), p(op, c_i32_p), p(of, c_i32_p), p(oxy, c_double_p))
    else:
        outs = (None, None, None, None)
    _lib.check(_lib.lib().ssfm_build_tracks_device(ctx._p, K, p(fptr, c_i32_p), p(fxy, c_double_p), len(i0), p(i0, c_i32_p), p(i1, c_i32_p), p(mptr, c_i32_p),
                                                   p(f0, c_i32_p), p(f1, c_i32_p), centerx, centery, p(tracks, c_i32_p), C.byref(npts), p(conflict, c_u8_p),
                                                   C.byref(nobs), *outs), ctx._p)
    n = nobs.value
    out = dict(tracks=tracks[:total], num_points=npts.value, conflict=conflict[:npts.value].astype(bool), num_observations=n,
               obs_cam=None, obs_pt=None, obs_feat=None, obs_xy=None)
    if observations:
        out.update(obs_cam=oc[:n], obs_pt=op[:n], obs_feat=of[:n], obs_xy=oxy[:n])
    return out


def build_tracks_device(ctx, features, image_matches, centerx=0.0, centery=0.0):
    """build_tracks(..., merge=True) as connected components on the device (ssfm_build_tracks_device): the same inputs.
    -> dict(tracks [list of int arrays per keyframe], num_points, conflict (bool per point), obs_cam, obs_pt, obs_feat, obs_xy); the ids are canonical
    (ascending smallest member) and the observations ordered by winning feature -- include/ssfm.h states where this and build_tracks agree."""
    fptr, fxy, i0, i1, mptr, f0, f1 = _flatten(features, image_matches)
    out = build_tracks_device_flat(ctx, fptr, fxy, i0, i1, mptr, f0, f1, centerx, centery)
    out["tracks"] = [out["tracks"][fptr[k]:fptr[k + 1]].copy() for k in range(len(features))]
    return out


def last_kernel_ms(ctx):
    """device time of the kernels of the context's last build_tracks_device call (ssfm_tracks_last_kernel_ms)"""
    ms = C.c_double(0)
    _lib.check(_lib.lib().ssfm_tracks_last_kernel_ms(ctx._p, C.byref(ms)), ctx._p)
    return ms.value
