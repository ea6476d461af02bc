"""GPU descriptor matching (ssfm_match_pairs / spherical_sfm_amd.match) against the numpy restatement tests/_match_ref.py of the reference's
match / match_exhaustive (examples/spherical_sfm_tools.cpp:235-251, :575-600).

Integer-valued descriptors (what OpenCV's SIFT stores: floats holding 0..255) are the contract: every squared distance is an integer below 2^24, so
the lists must be array_equal, no tolerance and no excluded case.  General float descriptors agree on every query whose ratio test is not decided
within 1e-5 (relative) in float64."""
import ctypes as C

import numpy as np
import pytest

import _match_ref as R
from spherical_sfm_amd import _lib, match, ransac, synth

pytestmark = pytest.mark.gpu

POOL = R.world_pool(8000, seed=1)


def _check_lists(got, want):
    assert np.array_equal(got["match_ptr"], want[0])
    assert np.array_equal(got["match_idx0"], want[1]) and np.array_equal(got["match_idx1"], want[2])


def _pass_fraction(frames, pairs, ratio=0.75):
    npass = nq = 0
    for a, b in pairs:
        nn, _, dist = R.knn2(frames[a], frames[b])
        npass += int(R.ratio_pass(dist, nn, ratio).sum()); nq += len(frames[b])
    return npass / max(nq, 1)


@pytest.mark.parametrize("n", [31, 500, 1000, 4000])
def test_integer_descriptors_exact_equal_sizes(gpu_ctx, n):
    frames = [R.integer_frame(POOL, n, 10 + n)[0], R.integer_frame(POOL, n, 11 + n)[0]]
    pairs = [(0, 1), (1, 0)]
    frac = _pass_fraction(frames, pairs)
    print(f"n={n}: {100 * frac:.1f} % of the queries pass the ratio test")
    got = match.match_pairs(gpu_ctx, frames, pairs)
    _check_lists(got, R.match_pairs(frames, pairs))
    assert 0.10 <= frac <= 0.90
    assert got["match_ptr"][-1] > 0


def test_integer_descriptors_exact_mixed_sizes(gpu_ctx):
    """frames of different sizes in one call: 0, 1 and 2 features, non-multiples of the tile edge, a frame matched with itself"""
    sizes = [500, 0, 1, 2, 31, 1000, 333, 129, 500]
    frames = [R.integer_frame(POOL, n, 50 + k, span=1000)[0] for k, n in enumerate(sizes)]
    pairs = R.exhaustive_pairs(len(sizes)) + [(5, 0), (4, 2), (3, 3), (1, 0), (0, 1), (2, 2)]
    frac = _pass_fraction(frames, pairs)
    print(f"mixed sizes: {100 * frac:.1f} % of the queries pass the ratio test")
    got = match.match_pairs(gpu_ctx, frames, pairs)
    want = R.match_pairs(frames, pairs)
    _check_lists(got, want)
    for p, (a, b) in enumerate(pairs):                       # per pair: ascending train index, each once; an empty list where the train frame has < 2 features
        j = got["match_idx0"][got["match_ptr"][p]:got["match_ptr"][p + 1]]
        assert (np.diff(j) > 0).all()
        if sizes[a] < 2:
            assert len(j) == 0
    assert 0.10 <= frac <= 0.90


def test_match_exhaustive_order(gpu_ctx):
    sizes = [200, 150, 260, 90]
    frames = [R.integer_frame(POOL, n, 80 + k, span=400)[0] for k, n in enumerate(sizes)]
    got = match.match_exhaustive(gpu_ctx, frames)
    pairs = R.exhaustive_pairs(4)
    assert list(zip(got["pair_frame0"].tolist(), got["pair_frame1"].tolist())) == pairs == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    _check_lists(got, R.match_pairs(frames, pairs))


@pytest.mark.parametrize("n0,n1", [(1000, 1000), (129, 517), (4000, 300), (2, 70), (1, 5), (0, 3)])
def test_knn_probe_integer(gpu_ctx, n0, n1):
    t = R.integer_frame(POOL, n0, 21 + n0, span=2 * max(n0, n1))[0]; q = R.integer_frame(POOL, n1, 22 + n1, span=2 * max(n0, n1))[0]
    nn, dist = match.knn_probe(gpu_ctx, t, q)
    rnn, rd2, rdist = R.knn2(t, q)
    assert np.array_equal(dist, rdist)                       # float distances, inf where there is no such row
    tie = rd2[:, 0] == rd2[:, 1]
    assert np.array_equal(nn[~tie], rnn[~tie])
    assert ((nn >= 0) == (rnn >= 0)).all()


def test_general_float_descriptors(gpu_ctx):
    ratio = 0.75
    sizes = [1000, 777, 1500]
    frames = [R.float_frame(POOL, n, 30 + k, span=2000)[0] for k, n in enumerate(sizes)]
    pairs = R.exhaustive_pairs(3) + [(2, 0)]
    got = match.match_pairs(gpu_ctx, frames, pairs, ratio=ratio)
    n_amb = n_all = 0
    for p, (a, b) in enumerate(pairs):
        rnn, rd2, rdist = R.knn2(frames[a], frames[b])
        amb = R.ambiguous(rd2, ratio); n_amb += int(amb.sum()); n_all += len(amb)
        rok = R.ratio_pass(rdist, rnn, ratio)
        nn, dist = match.knn_probe(gpu_ctx, frames[a], frames[b])
        gok = R.ratio_pass(dist, nn, ratio)
        keep = ~amb
        assert np.array_equal(gok[keep], rok[keep])                                   # the decision of every non-ambiguous query ...
        assert np.array_equal(nn[keep & rok, 0], rnn[keep & rok, 0])                  # ... and the train row it goes to
        # the lists: equal on every train row that no ambiguous query could have claimed
        touched = set(rnn[amb].ravel().tolist()) | set(nn[amb].ravel().tolist())
        j = got["match_idx0"][got["match_ptr"][p]:got["match_ptr"][p + 1]]; i = got["match_idx1"][got["match_ptr"][p]:got["match_ptr"][p + 1]]
        wj, wi = R.match_pair(frames[a], frames[b], ratio)
        g = {int(x): int(y) for x, y in zip(j, i) if int(x) not in touched}; w = {int(x): int(y) for x, y in zip(wj, wi) if int(x) not in touched}
        assert g == w
    print(f"float descriptors: {n_amb} ambiguous of {n_all} queries")
    assert n_amb <= 0.001 * n_all


def test_overwrite_rule_on_the_device(gpu_ctx):
    """three queries whose nearest train row is row 1: the largest query index stays"""
    t = np.zeros((3, 128), np.float32); t[0, 0] = 100; t[1, 1] = 100; t[2, 2] = 100
    q = np.zeros((5, 128), np.float32)
    q[0, 1] = 90; q[1, 0] = 95; q[2, 1] = 99; q[3, 2] = 50; q[3, 1] = 49; q[4, 1] = 80      # query 3: no clear winner
    got = match.match_pairs(gpu_ctx, [t, q], [(0, 1)])
    wj, wi = R.match_pair(t, q)
    assert wj.tolist() == [0, 1] and wi.tolist() == [1, 4]
    assert got["match_idx0"].tolist() == [0, 1] and got["match_idx1"].tolist() == [1, 4]


def test_exact_tie_goes_to_the_lower_train_index(gpu_ctx):
    t = np.zeros((200, 128), np.float32); t[:, 5] = 200.0                       # every row far from the query ...
    t[150, :] = 0; t[150, 0] = 10; t[37, :] = 0; t[37, 1] = 10                  # ... but two rows at exactly the same distance, in different tiles
    q = np.zeros((1, 128), np.float32)
    for ratio, want in ((0.75, []), (1.0, []), (1.5, [37])):
        got = match.match_pairs(gpu_ctx, [t, q], [(0, 1)], ratio=ratio)
        assert got["match_idx0"].tolist() == want, ratio
        assert R.match_pair(t, q, ratio)[0].tolist() == want
    nn, dist = match.knn_probe(gpu_ctx, t, q)
    assert nn.tolist() == [[37, 150]] and dist.tolist() == [[10.0, 10.0]]


def _raw_call(ctx, fp, d, f0, f1, opt, cap, mp, m0, m1, num_frames=None):
    fp = np.ascontiguousarray(fp, np.int32); d = np.ascontiguousarray(d, np.float32); f0 = np.ascontiguousarray(f0, np.int32); f1 = np.ascontiguousarray(f1, np.int32)
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None
    return _lib.lib().ssfm_match_pairs(ctx._p, len(fp) - 1 if num_frames is None else num_frames, p(fp, _lib.c_i32_p), p(d, _lib.c_float_p), len(f0), p(f0, _lib.c_i32_p),
                                       p(f1, _lib.c_i32_p), C.byref(opt) if opt is not None else None, C.c_int64(cap), p(mp, _lib.c_i32_p), p(m0, _lib.c_i32_p), p(m1, _lib.c_i32_p))


def test_capacity_protocol_and_argument_checks(gpu_ctx):
    frames = [R.integer_frame(POOL, n, 60 + k, span=300)[0] for k, n in enumerate([150, 140, 130])]
    pairs = R.exhaustive_pairs(3)
    fp, d, _ = match._flatten(frames)
    f0 = [a for a, _ in pairs]; f1 = [b for _, b in pairs]
    want = R.match_pairs(frames, pairs); total = int(want[0][-1]); assert total > 10
    o = match.default_options()
    assert (o.ratio, o.dim) == (0.75, 128)
    # NULL lists: counts only
    mp = np.zeros(4, np.int32)
    assert _raw_call(gpu_ctx, fp, d, f0, f1, o, 0, mp, None, None) == 0 and np.array_equal(mp, want[0])
    # too small: SSFM_ERR_INVALID and the needed total
    mp = np.zeros(4, np.int32); m0 = np.zeros(total, np.int32); m1 = np.zeros(total, np.int32)
    assert _raw_call(gpu_ctx, fp, d, f0, f1, o, total - 1, mp, m0, m1) == -1 and mp[-1] == total
    assert b"capacity" in _lib.lib().ssfm_last_error(gpu_ctx._p)
    # exactly enough
    assert _raw_call(gpu_ctx, fp, d, f0, f1, o, total, mp, m0, m1) == 0 and np.array_equal(m0, want[1]) and np.array_equal(m1, want[2])
    # refused before any launch
    bad = match.default_options(dim=130); assert _raw_call(gpu_ctx, fp, d, f0, f1, bad, total, mp, m0, m1) == -1
    bad = match.default_options(dim=6); assert _raw_call(gpu_ctx, fp, d, f0, f1, bad, total, mp, m0, m1) == -1
    bad = match.default_options(ratio=0.0); assert _raw_call(gpu_ctx, fp, d, f0, f1, bad, total, mp, m0, m1) == -1
    bad = match.default_options(ratio=float("nan")); assert _raw_call(gpu_ctx, fp, d, f0, f1, bad, total, mp, m0, m1) == -1
    assert _raw_call(gpu_ctx, fp, d, [0, 3], [1, 2], o, total, mp, m0, m1) == -1 and b"frame index" in _lib.lib().ssfm_last_error(gpu_ctx._p)
    assert _raw_call(gpu_ctx, fp, d, [0, -1], [1, 2], o, total, mp, m0, m1) == -1
    assert _raw_call(gpu_ctx, [0, 150, 140, 420], d, f0, f1, o, total, mp, m0, m1) == -1          # feat_ptr does not ascend
    assert _raw_call(gpu_ctx, fp, d, f0, f1, o, total, None, m0, m1) == -1
    assert _raw_call(gpu_ctx, fp, d, f0, f1, o, total, mp, m0, None) == -1
    assert _raw_call(gpu_ctx, fp, d, f0, f1, o, -1, mp, m0, m1) == -1
    with pytest.raises(_lib.SsfmError):
        match.match_pairs(gpu_ctx, frames, [(0, 7)])
    # a shorter descriptor length (multiple of 4): the same contract
    f32 = [f[:, :32].copy() for f in frames]
    _check_lists(match.match_pairs(gpu_ctx, f32, pairs), R.match_pairs(f32, pairs))
    f20 = [f[:, :20].copy() for f in frames]
    _check_lists(match.match_pairs(gpu_ctx, f20, pairs), R.match_pairs(f20, pairs))


def test_repeatability(gpu_ctx):
    sizes = [700, 650, 900, 300]
    frames = [R.integer_frame(POOL, n, 70 + k, span=1200)[0] for k, n in enumerate(sizes)]
    first = match.match_exhaustive(gpu_ctx, frames)
    assert first["match_ptr"][-1] > 100
    for _ in range(4):
        again = match.match_exhaustive(gpu_ctx, frames)
        for k in ("match_ptr", "match_idx0", "match_idx1"):
            assert np.array_equal(first[k], again[k])


def test_slabs(gpu_ctx, monkeypatch):
    """a call that crosses slab boundaries (SSFM_MATCH_SLAB_PAIRS is read at every call) equals the same pairs matched one per call"""
    sizes = [300, 250, 0, 310, 129, 200]
    frames = [R.integer_frame(POOL, n, 90 + k, span=500)[0] for k, n in enumerate(sizes)]
    pairs = R.exhaustive_pairs(len(sizes))                                            # 15 pairs
    whole = match.match_pairs(gpu_ctx, frames, pairs)
    monkeypatch.setenv("SSFM_MATCH_SLAB_PAIRS", "4")                                  # slabs of 4, 4, 4, 3
    slabbed = match.match_pairs(gpu_ctx, frames, pairs)
    monkeypatch.delenv("SSFM_MATCH_SLAB_PAIRS")
    ptr = [0]; a0 = []; a1 = []
    for pr in pairs:
        one = match.match_pairs(gpu_ctx, frames, [pr])
        a0.append(one["match_idx0"]); a1.append(one["match_idx1"]); ptr.append(ptr[-1] + len(one["match_idx0"]))
    for got in (whole, slabbed):
        assert np.array_equal(got["match_ptr"], np.array(ptr, np.int32))
        assert np.array_equal(got["match_idx0"], np.concatenate(a0)) and np.array_equal(got["match_idx1"], np.concatenate(a1))
    _check_lists(whole, R.match_pairs(frames, pairs))
    # the capacity protocol across slabs: the needed total is still reported
    monkeypatch.setenv("SSFM_MATCH_SLAB_PAIRS", "4")
    fp, d, _ = match._flatten(frames)
    mp = np.zeros(len(pairs) + 1, np.int32); m0 = np.zeros(5, np.int32); m1 = np.zeros(5, np.int32)
    assert _raw_call(gpu_ctx, fp, d, [a for a, _ in pairs], [b for _, b in pairs], None, 5, mp, m0, m1) == -1 and mp[-1] == ptr[-1]


def _two_view_frames(num_frames=3, n=260, seed=5):
    """Frames with feature rays AND descriptors: frame f holds the u rays of relative-pose problem f and, shuffled, the v rays of problem f - 1 (cyclic),
    so that two frames are two-view consistent on the features they share; descriptors of a shared feature are two noisy integer views of one
    world descriptor.  -> (feat_ptr, feat_rays, descs_per_frame)"""
    rng = np.random.default_rng(seed)
    probs = [synth.make_relative_pose_problem(n, seed=400 + f, noise=1 / 600, outlier_frac=0.2, rotation_deg=6 + f) for f in range(num_frames)]
    pool = R.world_pool(num_frames * n, seed=seed + 1)

    def view(ids, s):
        r = np.random.default_rng(s)
        v = np.maximum(pool[ids] * (1.0 + 0.15 * r.standard_normal((len(ids), 128))), 0.0)
        return np.clip(np.rint(v / np.linalg.norm(v, axis=1, keepdims=True) * 512.0), 0, 255).astype(np.float32)

    rays, descs = [], []
    for f in range(num_frames):
        ids_u = f * n + np.arange(n); r = [probs[f][0]]; d = [view(ids_u, 1000 + f)]
        g = (f - 1) % num_frames                                                 # (cyclic: every pair of the three frames shares one problem's features)
        perm = rng.permutation(n)
        r.append(probs[g][1][perm]); d.append(view(g * n + perm, 2000 + f))
        rays.append(np.concatenate(r)); descs.append(np.concatenate(d))
    feat_ptr = np.zeros(num_frames + 1, np.int32); feat_ptr[1:] = np.cumsum([len(r) for r in rays])
    return feat_ptr, np.ascontiguousarray(np.concatenate(rays)), descs


def test_match_lists_feed_ransac_unchanged(gpu_ctx):
    feat_ptr, feat_rays, descs = _two_view_frames()
    got = match.match_exhaustive(gpu_ctx, descs)
    want = R.match_pairs(descs, R.exhaustive_pairs(len(descs)))
    _check_lists(got, want)
    assert (np.diff(got["match_ptr"]) > 150).all()                               # every pair of frames shares 260 features
    assert np.array_equal(got["feat_ptr"], feat_ptr)
    kw = dict(min_num_inliers=20)
    a = ransac.estimate_indexed(gpu_ctx, feat_ptr, feat_rays, got["pair_frame0"], got["pair_frame1"], got["match_ptr"], got["match_idx0"], got["match_idx1"], (2 / 600) ** 2, **kw)
    pr = np.array(R.exhaustive_pairs(len(descs)), np.int32)
    b = ransac.estimate_indexed(gpu_ctx, feat_ptr, feat_rays, pr[:, 0], pr[:, 1], want[0], want[1], want[2], (2 / 600) ** 2, **kw)
    for k in ("E", "R", "mask", "num_inliers", "scores", "iterations", "lo_runs"):
        assert np.array_equal(a[k], b[k]), k
    assert a["num_inliers"][0] > 100 and a["num_inliers"][2] > 100             # the consistent pairs (0, 1) and (1, 2) are found


def test_last_kernel_ms(gpu_ctx):
    frames = [R.integer_frame(POOL, 1000, 5)[0], R.integer_frame(POOL, 1000, 6)[0]]
    match.match_pairs(gpu_ctx, frames, [(0, 1)])
    ms = match.last_kernel_ms(gpu_ctx)
    assert 0.0 < ms < 1000.0
