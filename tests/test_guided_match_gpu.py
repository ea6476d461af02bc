"""Guided matching on the GPU (ssfm_guided_match_pairs, ssfm_guided_knn_probe, pairwise.guided_rematch) against the numpy restatement tests/_guided_ref.py.
Integer descriptors throughout, so every distance is exact in float32 and the lists are compared with array_equal.  The fp64 predicate is compared exactly
as well: every fixture first asserts on the CPU that no (query, train) entry lies within 1e-9 (relative) of the band's edge -- ten thousand times the rounding
of a dozen fp64 operations in any order or contraction -- before the device is asked."""
import ctypes as C
import functools

import numpy as np
import pytest

import _front_scene as S
import _guided_ref as G
from spherical_sfm_amd import _lib, match, pairwise, ransac
from spherical_sfm_amd._lib import c_double_p, c_float_p, c_i32_p

pytestmark = pytest.mark.gpu
THR = G.THR2
GAP = 1e-9


def _gap_ok(u, v, E, thr2):
    if len(u) and len(v):
        assert G.band_gap(G.sampson(u, v, E), thr2) > GAP


@functools.lru_cache(maxsize=None)
def probe_scene(n0, n1, dim):
    """n0 train and n1 query features of a 4 degree pair: observations of the same world points (so the bands hold true matches and bystanders), a seventh of
    the points carrying the descriptor of their predecessor WITHOUT noise in the train frame (exact ties between candidates)"""
    rng = np.random.default_rng(1000 * n0 + n1 + dim)
    n = max(n0, n1)
    X, D = S._world(rng, n, 2.0 * np.pi / 180, dim)
    t = S._noisy(D, rng)[:n0].copy()
    t[1::7] = t[0::7][:len(t[1::7])]
    sel = rng.permutation(n)[:n1]
    q = S._noisy(D, rng)[sel]
    u = S.rays_of(S._project(X[:n0], 0.0, rng, 0.3)); v = S.rays_of(S._project(X[sel], 4.0 * np.pi / 180, rng, 0.3))
    return t, u, q, v, G.essential_of_step(4.0)[0]


@pytest.mark.parametrize("dim", [128, 32])
@pytest.mark.parametrize("n0,n1", [(1, 1), (2, 3), (127, 129), (128, 128), (129, 257), (300, 5), (5, 300)])
def test_probe_equals_the_restatement(gpu_ctx, n0, n1, dim):
    t, u, q, v, E = probe_scene(n0, n1, dim)
    for thr2 in (THR, 100.0 * THR):                                                  # 2 px: a few rows per band; 20 px: dozens, ties among them
        _gap_ok(u, v, E, thr2)
        nn, dist, cnt = G.knn2(t, u, q, v, E, thr2)
        gnn, gdist, gcnt = match.guided_knn_probe(gpu_ctx, t, u, q, v, E, thr2)
        assert np.array_equal(gcnt, cnt), (thr2, np.flatnonzero(gcnt != cnt))
        assert np.array_equal(gnn, nn), (thr2, np.flatnonzero((gnn != nn).any(1)))
        assert np.array_equal(gdist, dist)
    if n0 >= 128:
        assert cnt.max() >= 3 and (nn[:, 1] >= 0).any() and (nn[:, 0] < 0).sum() < n1     # the wide band really ranks: two finalists out of more candidates


def _pair_lists(mp, m0, m1, p):
    return m0[mp[p]:mp[p + 1]], m1[mp[p]:mp[p + 1]]


def _one_pair(ctx, sc, thr2, **kw):
    fp = np.array([0, len(sc["train"]), len(sc["train"]) + len(sc["query"])], np.int32)
    descs = np.concatenate([sc["train"], sc["query"]]); rays = np.concatenate([sc["u"], sc["v"]])
    return fp, descs, rays, match.guided_match_flat(ctx, fp, descs, rays, [0], [1], sc["E"][None], thr2, **kw)


@pytest.mark.parametrize("seed", range(4))
def test_repeated_structure_lists_equal_the_restatement_and_beat_the_plain_matcher(gpu_ctx, seed):
    sc = G.repeated_pair(seed)
    _gap_ok(sc["u"], sc["v"], sc["E"], THR)
    want = G.guided_pair(sc["train"], sc["u"], sc["query"], sc["v"], sc["E"], THR, 0.75)
    fp, descs, rays, (mp, m0, m1) = _one_pair(gpu_ctx, sc, THR)
    assert mp.tolist() == [0, len(want[0])] and np.array_equal(m0, want[0]) and np.array_equal(m1, want[1])
    pp, p0, p1 = match.match_flat(gpu_ctx, fp, descs, [0], [1], ratio=0.75)
    assert len(m0) >= 1.5 * len(p0) and len(p0) > 0
    assert np.array_equal(sc["truth"][m1], m0)                                       # all correct


def arc_scene():
    frames = S.arc_frames((130, 70, 130, 2, 70))
    fp, descs, rays = S.flatten(frames)
    pairs = np.array(match.exhaustive_pairs(len(frames)), np.int32)
    Es = np.stack([G.essential_of_step(4.0 * (b - a))[0] for a, b in pairs])
    return frames, fp, descs, rays, pairs, Es


def test_a_band_that_admits_everything_is_ssfm_match_pairs_bit_for_bit(gpu_ctx):
    frames, fp, descs, rays, pairs, Es = arc_scene()
    for ratio in (0.75, 1.0):
        plain = match.match_flat(gpu_ctx, fp, descs, pairs[:, 0], pairs[:, 1], ratio=ratio)
        guided = match.guided_match_flat(gpu_ctx, fp, descs, rays, pairs[:, 0], pairs[:, 1], Es, 1e30, ratio=ratio)
        assert plain[0][-1] > 100
        for a, b in zip(plain, guided):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_threshold_zero_and_zero_E_give_nothing(gpu_ctx):
    frames, fp, descs, rays, pairs, Es = arc_scene()
    for E, thr2 in ((Es, 0.0), (np.zeros_like(Es), THR), (np.zeros_like(Es), 1e30)):
        mp, m0, m1 = match.guided_match_flat(gpu_ctx, fp, descs, rays, pairs[:, 0], pairs[:, 1], E, thr2)
        assert not mp.any() and len(mp) == len(pairs) + 1 and len(m0) == 0 and len(m1) == 0


@functools.lru_cache(maxsize=None)
def six_pairs():
    """frames 0 (130) and 1 (70) twice under two different E's, pairs with the empty frame 2 on either side, and a train frame of ONE feature
    (frame 3) whose point frame 4 observes one step later as its last feature, so the pair with n0 = 1 does match"""
    frames = S.arc_frames((130, 70, 0, 1, 130), seed=7)
    rng = np.random.default_rng(8)
    X, D = S._world(rng, 1, 0.0, 128)
    frames[3] = (S._project(X, 0.0, rng, 0.3), S._noisy(D, rng))
    xy4, d4 = frames[4]
    frames[4] = (np.concatenate([xy4, S._project(X, 4.0 * np.pi / 180, rng, 0.3)]), np.concatenate([d4, S._noisy(D, rng)]))
    fp, descs, rays = S.flatten(frames)
    pairs = np.array([(0, 1), (0, 1), (0, 2), (2, 0), (3, 4), (1, 0)], np.int32)
    E4, E8 = G.essential_of_step(4.0)[0], G.essential_of_step(8.0)[0]
    Es = np.stack([E4, E8, E4, E4, E4, G.essential_of_step(-4.0)[0]])
    return frames, fp, descs, rays, pairs, Es


def test_six_pairs_in_one_call_slabs_and_repeats(gpu_ctx, monkeypatch):
    frames, fp, descs, rays, pairs, Es = six_pairs()
    thr2 = 4.0 * THR
    dl = [f[1] for f in frames]; rl = [S.rays_of(f[0]) for f in frames]
    for (a, b), E in zip(pairs, Es):
        _gap_ok(rl[a], rl[b], E, thr2)
    want = G.guided_pairs(dl, rl, pairs, Es, thr2)
    got = match.guided_match_flat(gpu_ctx, fp, descs, rays, pairs[:, 0], pairs[:, 1], Es, thr2)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    cnt = np.diff(got[0])
    assert cnt[0] > 10 and cnt[1] != cnt[0] and cnt[2] == 0 and cnt[3] == 0 and cnt[4] == 1 and cnt[5] > 10      # the lone train feature matches
    for p in range(len(pairs)):                                                      # every pair equals its single-pair call
        one = match.guided_match_flat(gpu_ctx, fp, descs, rays, pairs[p:p + 1, 0], pairs[p:p + 1, 1], Es[p:p + 1], thr2)
        assert np.array_equal(one[1], _pair_lists(*got, p)[0]) and np.array_equal(one[2], _pair_lists(*got, p)[1])
    with monkeypatch.context() as m:
        m.setenv("SSFM_MATCH_SLAB_PAIRS", "1")
        slab = match.guided_match_flat(gpu_ctx, fp, descs, rays, pairs[:, 0], pairs[:, 1], Es, thr2)
    again = match.guided_match_flat(gpu_ctx, fp, descs, rays, pairs[:, 0], pairs[:, 1], Es, thr2)
    for a, b, c in zip(got, slab, again):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    d = match.guided_match_pairs(gpu_ctx, dl, rl, pairs, Es, thr2)                   # the per-frame form
    assert np.array_equal(d["match_ptr"], got[0]) and np.array_equal(d["match_idx0"], got[1]) and np.array_equal(d["match_idx1"], got[2])
    assert match.guided_last_kernel_ms(gpu_ctx) > 0.0


def _raw(ctx, fp, descs, rays, f0, f1, E, o, cap, mp, m0, m1):
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None
    return _lib.lib().ssfm_guided_match_pairs(ctx._p, len(fp) - 1, p(fp, c_i32_p), p(descs, c_float_p), p(rays, c_double_p), len(f0), p(f0, c_i32_p), p(f1, c_i32_p),
                                              p(E, c_double_p), C.byref(o) if o is not None else None, C.c_int64(cap), p(mp, c_i32_p), p(m0, c_i32_p), p(m1, c_i32_p))


def _raw_args():
    frames, fp, descs, rays, pairs, Es = six_pairs()
    f0 = np.ascontiguousarray(pairs[:, 0]); f1 = np.ascontiguousarray(pairs[:, 1])
    return fp, descs, rays, f0, f1, match._flat_E(Es)


def test_capacity_protocol_and_counts_only(gpu_ctx):
    fp, descs, rays, f0, f1, E = _raw_args()
    o = match.guided_default_options(squared_threshold=4.0 * THR)
    full = match.guided_match_flat(gpu_ctx, fp, descs, rays, f0, f1, E.reshape(-1, 3, 3).transpose(0, 2, 1), 4.0 * THR)
    total = int(full[0][-1])
    mp = np.full(len(f0) + 1, -7, np.int32)
    assert _raw(gpu_ctx, fp, descs, rays, f0, f1, E, o, 0, mp, None, None) == 0 and np.array_equal(mp, full[0])              # NULL lists: counts only
    cnt, none0, none1 = match.guided_match_flat(gpu_ctx, fp, descs, rays, f0, f1, E.reshape(-1, 3, 3).transpose(0, 2, 1), 4.0 * THR, count_only=True)
    assert np.array_equal(cnt, full[0]) and none0 is None and none1 is None
    mp[:] = -7; m0 = np.zeros(total, np.int32); m1 = np.zeros(total, np.int32)
    rc = _raw(gpu_ctx, fp, descs, rays, f0, f1, E, o, total - 1, mp, m0, m1)
    assert rc != 0 and b"capacity too small" in _lib.lib().ssfm_last_error(gpu_ctx._p) and mp[-1] == total and np.array_equal(mp, full[0])
    assert _raw(gpu_ctx, fp, descs, rays, f0, f1, E, o, total, mp, m0, m1) == 0 and np.array_equal(m0, full[1]) and np.array_equal(m1, full[2])
    with pytest.raises(_lib.SsfmError, match="ssfm_guided_match_pairs: capacity too small"):
        match.guided_match_flat(gpu_ctx, fp, descs, rays, f0, f1, E.reshape(-1, 3, 3).transpose(0, 2, 1), 4.0 * THR, capacity=1)
    # no pairs, and frames without features
    mp, m0, m1 = match.guided_match_flat(gpu_ctx, fp, descs, rays, [], [], np.zeros((0, 3, 3)), THR)
    assert mp.tolist() == [0] and len(m0) == 0


def test_refused_arguments_return_before_any_launch(gpu_ctx):
    fp, descs, rays, f0, f1, E = _raw_args()
    P = len(f0)
    good = lambda **kw: match.guided_default_options(**{"squared_threshold": THR, **kw})
    mp = np.zeros(P + 1, np.int32); m0 = np.zeros(1000, np.int32); m1 = np.zeros(1000, np.int32)
    assert _raw(gpu_ctx, fp, descs, rays, f0, f1, E, good(), 1000, mp, m0, m1) == 0
    ms = match.guided_last_kernel_ms(gpu_ctx)
    assert ms > 0.0
    bad_f = f0.copy(); bad_f[2] = 99
    bad_fp = fp.copy(); bad_fp[2] = bad_fp[1] - 1
    cases = [
        ((fp, descs, rays, f0, f1, None, good(), 1000, mp, m0, m1), "E is null"),
        ((fp, descs, None, f0, f1, E, good(), 1000, mp, m0, m1), "feat_rays is null"),
        ((fp, None, rays, f0, f1, E, good(), 1000, mp, m0, m1), "descs is null"),
        ((fp, descs, rays, f0, f1, E, good(squared_threshold=-1e-9), 1000, mp, m0, m1), "squared_threshold must be >= 0"),
        ((fp, descs, rays, f0, f1, E, good(squared_threshold=np.nan), 1000, mp, m0, m1), "squared_threshold must be >= 0"),
        ((fp, descs, rays, f0, f1, E, good(max_distance=-1.0), 1000, mp, m0, m1), "max_distance must be >= 0"),
        ((fp, descs, rays, f0, f1, E, good(max_distance=np.nan), 1000, mp, m0, m1), "max_distance must be >= 0"),
        ((fp, descs, rays, f0, f1, E, good(dim=6), 1000, mp, m0, m1), "dim must be a multiple of 4 in 4..128"),
        ((fp, descs, rays, f0, f1, E, good(dim=132), 1000, mp, m0, m1), "dim must be a multiple of 4 in 4..128"),
        ((fp, descs, rays, f0, f1, E, good(ratio=0.0), 1000, mp, m0, m1), "ratio must be positive and finite"),
        ((fp, descs, rays, bad_f, f1, E, good(), 1000, mp, m0, m1), "frame index out of range"),
        ((bad_fp, descs, rays, f0, f1, E, good(), 1000, mp, m0, m1), "feat_ptr must ascend"),
        ((fp, descs, rays, f0, None, E, good(), 1000, mp, m0, m1), "bad arguments"),
        ((fp, descs, rays, f0, f1, E, good(), 1000, None, m0, m1), "bad arguments"),
        ((fp, descs, rays, f0, f1, E, good(), -1, mp, m0, m1), "bad arguments"),
        ((fp, descs, rays, f0, f1, E, good(), 1000, mp, m0, None), "given together or not at all"),
    ]
    for args, text in cases:
        rc = _raw(gpu_ctx, *args)
        msg = _lib.lib().ssfm_last_error(gpu_ctx._p).decode()
        assert rc != 0, text
        assert msg.startswith("ssfm_guided_match_pairs: ") and text in msg, (text, msg)
        assert match.guided_last_kernel_ms(gpu_ctx) == ms                            # the slab loop, which resets the time before its first launch, was not entered
    assert _lib.lib().ssfm_guided_match_pairs(None, 1, None, None, None, 0, None, None, None, None, 0, None, None, None) != 0
    # the probe's own checks
    t, u, q, v, Ep = probe_scene(2, 3, 32)
    with pytest.raises(_lib.SsfmError, match="ssfm_guided_knn_probe: squared_threshold must be >= 0"):
        match.guided_knn_probe(gpu_ctx, t, u, q, v, Ep, -1.0)
    with pytest.raises(_lib.SsfmError, match="ssfm_guided_knn_probe: dim must be a multiple of 4"):
        match.guided_knn_probe(gpu_ctx, t[:, :6], u, q[:, :6], v, Ep, THR)
    # a context with a communicator
    from spherical_sfm_amd import ba
    ctx = ba.Context(0)
    try:
        hook = _lib.HOST_ALLREDUCE_FN(lambda user, buf, n, op: 0)
        _lib.check(_lib.lib().ssfm_comm_init_host(ctx._p, 1, 0, hook, None), ctx._p)
        assert _raw(ctx, fp, descs, rays, f0, f1, E, good(), 1000, mp, m0, m1) != 0
        assert "ssfm_guided_match_pairs: the context carries a communicator" in _lib.lib().ssfm_last_error(ctx._p).decode()
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def ring_scene():
    frames = S.ring_frames(12, 60)
    fp, descs, rays = S.flatten(frames)
    return frames, fp, descs, rays, match.exhaustive_pairs(len(frames))


def _check_rematch(frames, pairs, res, out, Es):
    assert np.array_equal(out.accepted_pair, res.accepted_pair) and np.array_equal(out.R, res.R) and len(out.inl_ptr) == len(res.accepted_pair) + 1
    assert np.array_equal(out.num_inliers, np.diff(out.inl_ptr))
    more = 0
    for a, p in enumerate(res.accepted_pair):
        f0, f1 = pairs[p]
        t, q = frames[f0][1], frames[f1][1]; u, v = S.rays_of(frames[f0][0]), S.rays_of(frames[f1][0])
        want = G.guided_pair(t, u, q, v, Es[a], THR, 0.75)
        j, i = out.matches(a)
        assert np.array_equal(j, want[0]) and np.array_equal(i, want[1]), (a, p)
        Sv = G.sampson(u, v, Es[a])
        assert (Sv[i, j] < THR).all() and len(np.unique(j)) == len(j) and len(np.unique(i)) == len(i) and (np.diff(j) > 0).all()
        more += len(j) >= len(res.matches(a)[0])
    assert more >= 0.9 * len(res.accepted_pair)                                      # (a verified inlier is inside the band; guided lists are rarely shorter)


def test_guided_rematch_of_the_spherical_front_end(gpu_ctx):
    frames, fp, descs, rays, pairs = ring_scene()
    res = pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ransac.default_options(min_num_inliers=10), sq_thresh=THR)
    assert len(res.accepted_pair) >= 12
    Es = pairwise.spherical_essential(res.R)
    for a, p in enumerate(res.accepted_pair):
        _gap_ok(S.rays_of(frames[pairs[p][0]][0]), S.rays_of(frames[pairs[p][1]][0]), Es[a], THR)
    out = pairwise.guided_rematch(gpu_ctx, descs, rays, fp, pairs, res, THR)
    _check_rematch(frames, pairs, res, out, Es)


def test_guided_rematch_of_the_five_point_front_end_checks_the_convention_of_E(gpu_ctx):
    """the E that ssfm_pairwise5_from_features returns is used as it comes: were it the transpose, the verified inliers would lie outside its band"""
    frames, fp, descs, rays, pairs = ring_scene()
    res = pairwise.pairwise5_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ransac.default_options(min_num_inliers=10), sq_thresh=THR, want_E=True)
    assert len(res.accepted_pair) >= 12 and res.E is not None
    for a, p in enumerate(res.accepted_pair):
        u, v = S.rays_of(frames[pairs[p][0]][0]), S.rays_of(frames[pairs[p][1]][0])
        _gap_ok(u, v, res.E[a], THR)
        j, i = res.matches(a)
        assert (G.sampson(u, v, res.E[a])[i, j] < THR).mean() > 0.9                  # v^T E u: the call's own inliers are inside the band of its E
        assert (G.sampson(u, v, res.E[a].T)[i, j] < THR).mean() < 0.5                # ... and not inside that of the transpose
    out = pairwise.guided_rematch(gpu_ctx, descs, rays, fp, pairs, res, THR)
    _check_rematch(frames, pairs, res, out, res.E)
    assert np.array_equal(out.E, res.E) and np.array_equal(out.t, res.t)
