"""Python host side of the brute-force descriptor matching (include/ssfm.h: ssfm_match_pairs) and of guided matching (ssfm_guided_match_pairs).
Mirrors match / match_exhaustive (examples/spherical_sfm_tools.cpp:235-251, :575-600): train = the first frame of a pair, query = the second."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import GuidedMatchOptionsC, MatchOptionsC, c_double_p, c_float_p, c_i32_p


def default_options(**kw):
    o = MatchOptionsC()
    _lib.lib().ssfm_match_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _flatten(descs_per_frame, dim=None):
    """-> (feat_ptr [F+1] int32, descs [total, dim] float32, dim)"""
    ds = [np.asarray(d, np.float32) for d in descs_per_frame]
    if dim is None:
        dims = {d.shape[1] for d in ds if d.ndim == 2 and d.shape[0] > 0}
        if len(dims) > 1:
            raise ValueError(f"frames with different descriptor lengths: {sorted(dims)}")
        dim = dims.pop() if dims else 128
    ds = [d.reshape(-1, dim) for d in ds]
    ptr = np.zeros(len(ds) + 1, np.int32)
    ptr[1:] = np.cumsum([len(d) for d in ds])
    flat = np.ascontiguousarray(np.concatenate(ds) if len(ds) else np.zeros((0, dim), np.float32), np.float32)
    return ptr, flat, dim


def match_flat(ctx, feat_ptr, descs, pair_frame0, pair_frame1, ratio=0.75, capacity=None, count_only=False):
    """The C call itself.  -> (match_ptr [P+1], match_idx0, match_idx1): the arguments of ransac.estimate_indexed.
    capacity=None: one counting call sizes the lists, a second one fills them.  count_only: (match_ptr, None, None)."""
    fp = np.ascontiguousarray(feat_ptr, np.int32); d = np.ascontiguousarray(descs, np.float32)
    f0 = np.ascontiguousarray(pair_frame0, np.int32); f1 = np.ascontiguousarray(pair_frame1, np.int32)
    if len(f0) != len(f1):
        raise ValueError("pair_frame0 and pair_frame1 differ in length")
    dim = d.shape[1] if d.ndim == 2 else 128
    o = default_options(ratio=ratio, dim=dim)
    P = len(f0)
    mp = np.zeros(P + 1, np.int32)
    fn = _lib.lib().ssfm_match_pairs

    def call(cap, m0, m1):
        return fn(ctx._p, len(fp) - 1, fp.ctypes.data_as(c_i32_p), d.ctypes.data_as(c_float_p), P, f0.ctypes.data_as(c_i32_p), f1.ctypes.data_as(c_i32_p),
                  C.byref(o), C.c_int64(cap), mp.ctypes.data_as(c_i32_p), m0.ctypes.data_as(c_i32_p) if m0 is not None else None,
                  m1.ctypes.data_as(c_i32_p) if m1 is not None else None)

    if count_only:
        _lib.check(call(0, None, None), ctx._p)
        return mp, None, None
    if capacity is None:                       # a pair has at most min(n0, n1) matches
        n = np.diff(fp)
        in_range = P and f0.min() >= 0 and f1.min() >= 0 and max(f0.max(), f1.max()) < len(n)      # (otherwise the call itself refuses the pair list)
        capacity = int(np.minimum(n[f0], n[f1]).sum()) if in_range else 0
    m0 = np.zeros(max(int(capacity), 1), np.int32); m1 = np.zeros(max(int(capacity), 1), np.int32)
    _lib.check(call(int(capacity), m0, m1), ctx._p)
    return mp, m0[:mp[-1]].copy(), m1[:mp[-1]].copy()


def match_pairs(ctx, descs_per_frame, pairs, ratio=0.75):
    """descs_per_frame: list of (n_f, dim) arrays; pairs: list of (frame0, frame1).  -> dict(pair_frame0, pair_frame1, match_ptr, match_idx0,
    match_idx1, feat_ptr): pair p matches feature match_idx0[k] of frame0 (train) with feature match_idx1[k] of frame1 (query), idx0 ascending."""
    fp, d, _ = _flatten(descs_per_frame)
    pr = np.asarray(pairs, np.int32).reshape(-1, 2)
    mp, m0, m1 = match_flat(ctx, fp, d, pr[:, 0], pr[:, 1], ratio=ratio)
    return dict(pair_frame0=pr[:, 0].copy(), pair_frame1=pr[:, 1].copy(), match_ptr=mp, match_idx0=m0, match_idx1=m1, feat_ptr=fp)


def exhaustive_pairs(num_frames):
    """every index0 < index1 in the reference's nested order (spherical_sfm_tools.cpp:577-586)"""
    return [(a, b) for a in range(num_frames) for b in range(a + 1, num_frames)]


def match_exhaustive(ctx, descs_per_frame, ratio=0.75):
    return match_pairs(ctx, descs_per_frame, exhaustive_pairs(len(descs_per_frame)), ratio=ratio)


def knn_probe(ctx, train, query):
    """per query the two nearest train rows and their float distances as the device computes them -> (nn (n1, 2) int32, dist (n1, 2) float32);
    -1 / inf where the train set has no such row"""
    t = np.ascontiguousarray(train, np.float32); q = np.ascontiguousarray(query, np.float32)
    dim = q.shape[1] if q.ndim == 2 else t.shape[1]
    t = t.reshape(-1, dim); q = q.reshape(-1, dim)
    nn = np.zeros((max(len(q), 1), 2), np.int32); dist = np.zeros((max(len(q), 1), 2), np.float32)
    _lib.check(_lib.lib().ssfm_match_knn_probe(ctx._p, len(t), t.ctypes.data_as(c_float_p), len(q), q.ctypes.data_as(c_float_p), dim,
                                               nn.ctypes.data_as(c_i32_p), dist.ctypes.data_as(c_float_p)), ctx._p)
    return nn[:len(q)], dist[:len(q)]


def guided_default_options(**kw):
    o = GuidedMatchOptionsC()
    _lib.lib().ssfm_guided_match_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _flat_E(E):
    """(P, 3, 3) matrices, v^T E u = 0 -> [9 P] column-major doubles"""
    return np.ascontiguousarray(np.transpose(np.asarray(E, np.float64).reshape(-1, 3, 3), (0, 2, 1))).reshape(-1)


def guided_match_flat(ctx, feat_ptr, descs, rays, pair_frame0, pair_frame1, E, squared_threshold, ratio=0.75, max_distance=np.inf, capacity=None, count_only=False):
    """The C call itself (ssfm_guided_match_pairs): match_flat with the rays (total, 3) of all features and one E (3, 3) per pair, v^T E u = 0 with u in
    frame0.  -> (match_ptr [P+1], match_idx0, match_idx1).  capacity=None: the bound that cannot miss, min(n0, n1) per pair."""
    fp = np.ascontiguousarray(feat_ptr, np.int32); d = np.ascontiguousarray(descs, np.float32); r = np.ascontiguousarray(rays, np.float64)
    f0 = np.ascontiguousarray(pair_frame0, np.int32); f1 = np.ascontiguousarray(pair_frame1, np.int32)
    if len(f0) != len(f1):
        raise ValueError("pair_frame0 and pair_frame1 differ in length")
    e = _flat_E(E)
    if len(e) != 9 * len(f0):
        raise ValueError("one 3 x 3 matrix per pair")
    if r.size != 3 * len(d):
        raise ValueError("one ray per descriptor")
    dim = d.shape[1] if d.ndim == 2 else 128
    o = guided_default_options(ratio=ratio, squared_threshold=squared_threshold, max_distance=max_distance, dim=dim)
    P = len(f0)
    mp = np.zeros(P + 1, np.int32)
    fn = _lib.lib().ssfm_guided_match_pairs

    def call(cap, m0, m1):
        return fn(ctx._p, len(fp) - 1, fp.ctypes.data_as(c_i32_p), d.ctypes.data_as(c_float_p), r.ctypes.data_as(c_double_p), P, f0.ctypes.data_as(c_i32_p),
                  f1.ctypes.data_as(c_i32_p), e.ctypes.data_as(c_double_p), C.byref(o), C.c_int64(cap), mp.ctypes.data_as(c_i32_p),
                  m0.ctypes.data_as(c_i32_p) if m0 is not None else None, m1.ctypes.data_as(c_i32_p) if m1 is not None else None)

    if count_only:
        _lib.check(call(0, None, None), ctx._p)
        return mp, None, None
    if capacity is None:
        n = np.diff(fp)
        in_range = P and f0.min() >= 0 and f1.min() >= 0 and max(f0.max(), f1.max()) < len(n)      # (otherwise the call itself refuses the pair list)
        capacity = int(np.minimum(n[f0], n[f1]).sum()) if in_range else 0
    m0 = np.zeros(max(int(capacity), 1), np.int32); m1 = np.zeros(max(int(capacity), 1), np.int32)
    _lib.check(call(int(capacity), m0, m1), ctx._p)
    return mp, m0[:mp[-1]].copy(), m1[:mp[-1]].copy()


def guided_match_pairs(ctx, descs_per_frame, rays_per_frame, pairs, E, squared_threshold, ratio=0.75, max_distance=np.inf):
    """match_pairs under one essential matrix per pair: descs_per_frame / rays_per_frame are lists of (n_f, dim) / (n_f, 3) arrays, E (P, 3, 3).
    -> the dict of match_pairs"""
    fp, d, _ = _flatten(descs_per_frame)
    rs = [np.asarray(r, np.float64).reshape(-1, 3) for r in rays_per_frame]
    r = np.concatenate(rs) if rs else np.zeros((0, 3))
    pr = np.asarray(pairs, np.int32).reshape(-1, 2)
    mp, m0, m1 = guided_match_flat(ctx, fp, d, r, pr[:, 0], pr[:, 1], E, squared_threshold, ratio=ratio, max_distance=max_distance)
    return dict(pair_frame0=pr[:, 0].copy(), pair_frame1=pr[:, 1].copy(), match_ptr=mp, match_idx0=m0, match_idx1=m1, feat_ptr=fp)


def guided_knn_probe(ctx, train, u, query, v, E, squared_threshold):
    """per query the two nearest train rows AMONG those inside its epipolar band, their float distances and the size of the band
    -> (nn (n1, 2) int32, dist (n1, 2) float32, cand_count (n1,) int32); -1 / inf where there is no such row"""
    t = np.ascontiguousarray(train, np.float32); q = np.ascontiguousarray(query, np.float32)
    dim = q.shape[1] if q.ndim == 2 else t.shape[1]
    t = t.reshape(-1, dim); q = q.reshape(-1, dim)
    uu = np.ascontiguousarray(u, np.float64).reshape(-1, 3); vv = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
    if len(uu) != len(t) or len(vv) != len(q):
        raise ValueError("one ray per descriptor")
    e = _flat_E(E)
    nn = np.zeros((max(len(q), 1), 2), np.int32); dist = np.zeros((max(len(q), 1), 2), np.float32); cnt = np.zeros(max(len(q), 1), np.int32)
    _lib.check(_lib.lib().ssfm_guided_knn_probe(ctx._p, len(t), t.ctypes.data_as(c_float_p), uu.ctypes.data_as(c_double_p), len(q), q.ctypes.data_as(c_float_p),
                                                vv.ctypes.data_as(c_double_p), dim, e.ctypes.data_as(c_double_p), C.c_double(squared_threshold),
                                                nn.ctypes.data_as(c_i32_p), dist.ctypes.data_as(c_float_p), cnt.ctypes.data_as(c_i32_p)), ctx._p)
    return nn[:len(q)], dist[:len(q)], cnt[:len(q)]


def guided_last_kernel_ms(ctx):
    """device time of the kernels of the context's last guided match call (ssfm_guided_match_last_kernel_ms)"""
    ms = C.c_double(0)
    _lib.check(_lib.lib().ssfm_guided_match_last_kernel_ms(ctx._p, C.byref(ms)), ctx._p)
    return ms.value


def last_kernel_ms(ctx):
    """device time of the kernels of the context's last match call (ssfm_match_last_kernel_ms)"""
    ms = C.c_double(0)
    _lib.check(_lib.lib().ssfm_match_last_kernel_ms(ctx._p, C.byref(ms)), ctx._p)
    return ms.value
