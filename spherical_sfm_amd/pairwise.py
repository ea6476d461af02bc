"""Python host side of the pairwise front end (include/ssfm.h: ssfm_pairwise_from_features, ssfm_pairwise5_from_features): match_exhaustive +
estimate_pairwise or estimate_pairwise_five_point (examples/spherical_sfm_tools.cpp:575-600, :309-420, :433-573) in one call, the match lists staying on the
device between the two stages."""
import ctypes as C
import numpy as np
from . import _lib, match as _match, ransac as _ransac
from ._lib import c_double_p, c_float_p, c_i32_p, c_i64_p, c_u32_p


class PairwiseResult:
    """accepted_pair [A] (indices into `pairs`, ascending), R (A, 3, 3), num_inliers [A], inl_ptr [A + 1], inl_idx0 / inl_idx1 (features of frame0 / frame1 of
    the inlier matches, ascending idx0 per pair); per input pair: match_count, num_inliers_all (-1: no candidate), iterations, lo_runs.
    pairwise5_from_features adds t (A, 3) and E (A, 3, 3) (None where E was not asked for)."""
    __slots__ = ("accepted_pair", "R", "t", "E", "num_inliers", "inl_ptr", "inl_idx0", "inl_idx1", "match_count", "num_inliers_all", "iterations", "lo_runs", "calls")

    def matches(self, a):
        """(idx0, idx1) of accepted pair a"""
        return self.inl_idx0[self.inl_ptr[a]:self.inl_ptr[a + 1]], self.inl_idx1[self.inl_ptr[a]:self.inl_ptr[a + 1]]


def _raw(five, ctx, feat_ptr, descs, rays, f0, f1, mo, ro, sq_thresh, pair_capacity, inlier_capacity, want_E=True):
    """One C call of either kind with the given capacities -> (rc, needed [2], acc, R, nin, ptr, i0, i1, mc, nall, st) + (t, E) for the five-point call"""
    P = len(f0)
    acc = np.zeros(max(pair_capacity, 1), np.int32); R = np.zeros(9 * max(pair_capacity, 1)); nin = np.zeros(max(pair_capacity, 1), np.int32)
    ptr = np.zeros(pair_capacity + 1, np.int32); i0 = np.zeros(max(inlier_capacity, 1), np.int32); i1 = np.zeros(max(inlier_capacity, 1), np.int32)
    need = np.zeros(2, np.int64); mc = np.zeros(max(P, 1), np.int32); nall = np.zeros(max(P, 1), np.int32); st = np.zeros(2 * max(P, 1), np.uint32)
    t = np.zeros(3 * max(pair_capacity, 1)); E = np.zeros(9 * max(pair_capacity, 1)) if want_E else None
    pose = (R.ctypes.data_as(c_double_p),) + ((t.ctypes.data_as(c_double_p), E.ctypes.data_as(c_double_p) if want_E else None) if five else ())
    fn = _lib.lib().ssfm_pairwise5_from_features if five else _lib.lib().ssfm_pairwise_from_features
    rc = fn(ctx._p, len(feat_ptr) - 1, feat_ptr.ctypes.data_as(c_i32_p), descs.ctypes.data_as(c_float_p), rays.ctypes.data_as(c_double_p), P,
            f0.ctypes.data_as(c_i32_p), f1.ctypes.data_as(c_i32_p), C.byref(mo), C.byref(ro), C.c_double(sq_thresh), C.c_int64(pair_capacity), C.c_int64(inlier_capacity),
            need.ctypes.data_as(c_i64_p), acc.ctypes.data_as(c_i32_p), *pose, nin.ctypes.data_as(c_i32_p), ptr.ctypes.data_as(c_i32_p),
            i0.ctypes.data_as(c_i32_p), i1.ctypes.data_as(c_i32_p), mc.ctypes.data_as(c_i32_p), nall.ctypes.data_as(c_i32_p), st.ctypes.data_as(c_u32_p))
    return (rc, need, acc, R, nin, ptr, i0, i1, mc[:P], nall[:P], st[:2 * P]) + ((t, E) if five else ())


def _front(five, ctx, descs, rays, feat_ptr, pairs, match_options, ransac_options, sq_thresh, pair_capacity, inlier_capacity, want_E=True):
    fp = np.ascontiguousarray(feat_ptr, np.int32); d = np.ascontiguousarray(descs, np.float32); r = np.ascontiguousarray(rays, np.float64)
    pr = np.asarray(pairs, np.int32).reshape(-1, 2)
    f0 = np.ascontiguousarray(pr[:, 0]); f1 = np.ascontiguousarray(pr[:, 1])
    mo = match_options or _match.default_options(dim=d.shape[1] if d.ndim == 2 and d.shape[1] else 128)
    ro = ransac_options or _ransac.default_options()
    P = len(f0); n = np.diff(fp)
    in_range = P and f0.min() >= 0 and f1.min() >= 0 and max(f0.max(), f1.max()) < len(n)          # (otherwise the call itself refuses the pair list)
    if pair_capacity is None:
        pair_capacity = P
    if inlier_capacity is None:
        inlier_capacity = int(np.minimum(n[f0], n[f1]).sum()) if in_range else 0
    calls = 1
    out = _raw(five, ctx, fp, d, r, f0, f1, mo, ro, sq_thresh, int(pair_capacity), int(inlier_capacity), want_E)
    if out[0] != 0 and (out[1][0] > pair_capacity or out[1][1] > inlier_capacity):
        calls = 2
        out = _raw(five, ctx, fp, d, r, f0, f1, mo, ro, sq_thresh, int(out[1][0]), int(out[1][1]), want_E)
    _lib.check(out[0], ctx._p)
    _, need, acc, R, nin, ptr, i0, i1, mc, nall, st = out[:11]
    A, T = int(need[0]), int(need[1])
    res = PairwiseResult()
    res.accepted_pair = acc[:A].copy(); res.R = _ransac._unflat(R[:9 * A]); res.num_inliers = nin[:A].copy(); res.inl_ptr = ptr[:A + 1].copy()
    res.inl_idx0 = i0[:T].copy(); res.inl_idx1 = i1[:T].copy(); res.match_count = mc.copy(); res.num_inliers_all = nall.copy()
    res.iterations = st[0::2].copy(); res.lo_runs = st[1::2].copy(); res.calls = calls
    if five:
        res.t = out[11][:3 * A].reshape(A, 3).copy(); res.E = _ransac._unflat(out[12][:9 * A]) if want_E else None
    return res


def pairwise_from_features_raw(ctx, feat_ptr, descs, rays, f0, f1, mo, ro, sq_thresh, pair_capacity, inlier_capacity):
    """One C call with the given capacities -> (rc, needed [2], arrays...) without raising on a capacity miss."""
    return _raw(False, ctx, feat_ptr, descs, rays, f0, f1, mo, ro, sq_thresh, pair_capacity, inlier_capacity)


def pairwise_from_features(ctx, descs, rays, feat_ptr, pairs, match_options=None, ransac_options=None, sq_thresh=(2.0 / 600) ** 2, pair_capacity=None,
                           inlier_capacity=None):
    """descs (total, dim) float32 and rays (total, 3) float64 of all frames' features, frame f owning rows feat_ptr[f] .. feat_ptr[f + 1]; pairs: (P, 2) frame
    indices (train, query).  Capacity protocol: the default capacities are the bounds that cannot miss (every pair accepted, min(n0, n1) inlier matches
    each: 8 bytes of host memory per possible match); with smaller ones given, a miss costs one retry of the WHOLE call with the sizes the library asks for.
    -> PairwiseResult"""
    return _front(False, ctx, descs, rays, feat_ptr, pairs, match_options, ransac_options, sq_thresh, pair_capacity, inlier_capacity)


def pairwise5_from_features_raw(ctx, feat_ptr, descs, rays, f0, f1, mo, ro, sq_thresh, pair_capacity, inlier_capacity, want_E=True):
    """One C call of ssfm_pairwise5_from_features -> the tuple of pairwise_from_features_raw + (t, E); E is None with want_E=False (the call gets NULL)."""
    return _raw(True, ctx, feat_ptr, descs, rays, f0, f1, mo, ro, sq_thresh, pair_capacity, inlier_capacity, want_E)


def pairwise5_from_features(ctx, descs, rays, feat_ptr, pairs, match_options=None, ransac_options=None, sq_thresh=(2.0 / 600) ** 2, pair_capacity=None,
                            inlier_capacity=None, want_E=True):
    """pairwise_from_features with general relative pose (five-point LO-MSAC, ransac.ransac5_batch_indexed) as the estimator: the same arguments, capacity
    defaults and one retry; the options fields the five-point estimator ignores are those of ssfm_ransac5_batch.
    -> PairwiseResult with t (A, 3) and E (A, 3, 3) (None with want_E=False)"""
    return _front(True, ctx, descs, rays, feat_ptr, pairs, match_options, ransac_options, sq_thresh, pair_capacity, inlier_capacity, want_E)


def spherical_essential(R, inward=False):
    """make_spherical_essential_matrix (src/spherical_utils.cpp:9-14): E = [t]x R with t = R e_z - e_z, negated if inward -- the arithmetic of the device's
    make_E_dev.  R (3, 3) or (A, 3, 3) -> E of the same shape, v^T E u = 0 for u in frame0 and v in frame1."""
    R = np.asarray(R, np.float64)
    Rs = R.reshape(-1, 3, 3)
    E = np.zeros_like(Rs)
    for a, Ra in enumerate(Rs):
        t = np.array([Ra[0, 2], Ra[1, 2], Ra[2, 2] - 1.0])
        if inward:
            t = -t
        E[a, 0] = t[1] * Ra[2] - t[2] * Ra[1]; E[a, 1] = t[2] * Ra[0] - t[0] * Ra[2]; E[a, 2] = t[0] * Ra[1] - t[1] * Ra[0]
    return E.reshape(R.shape)


def guided_rematch(ctx, descs, rays, feat_ptr, pairs, result, sq_thresh, inward=False, ratio=0.75, max_distance=np.inf):
    """Guided matching (match.guided_match_flat) of the ACCEPTED pairs of a PairwiseResult under their own essential matrices: result.E where the
    result carries one (pairwise5_from_features with want_E), otherwise spherical_essential(result.R, inward).  -> a PairwiseResult with the same
    accepted pairs, poses and per-pair statistics whose inlier lists (inl_ptr, inl_idx0, inl_idx1, num_inliers) are the guided lists."""
    pr = np.asarray(pairs, np.int32).reshape(-1, 2)[result.accepted_pair]
    E = result.E if getattr(result, "E", None) is not None else spherical_essential(result.R, inward)
    mp, m0, m1 = _match.guided_match_flat(ctx, feat_ptr, descs, rays, pr[:, 0], pr[:, 1], np.asarray(E).reshape(-1, 3, 3), sq_thresh, ratio=ratio, max_distance=max_distance)
    out = PairwiseResult()
    for k in PairwiseResult.__slots__:
        if hasattr(result, k):
            setattr(out, k, getattr(result, k))
    out.inl_ptr = mp; out.inl_idx0 = m0; out.inl_idx1 = m1; out.num_inliers = np.diff(mp).astype(np.int32)
    return out


def last_kernel_ms(ctx):
    """device time of the kernels of the context's last pairwise_from_features / pairwise5_from_features call (ssfm_pairwise_front_last_kernel_ms)"""
    ms = C.c_double(0)
    _lib.check(_lib.lib().ssfm_pairwise_front_last_kernel_ms(ctx._p, C.byref(ms)), ctx._p)
    return ms.value
