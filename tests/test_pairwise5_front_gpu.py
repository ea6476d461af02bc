"""ssfm_pairwise5_from_features on the GPU: the call is DEFINED as the composition ssfm_match_pairs -> candidates -> ssfm_ransac5_batch_indexed -> acceptance,
so every output (t and E included) is compared array_equal with that composition computed here from the two existing wrappers; one scene is also held against
the numpy matcher (tests/_match_ref.py) and the numpy restatement of the five-point LO-MSAC (tests/fivepoint_ref.py).
TOL is SOLVER_TOL of tests/test_fivepoint_gpu.py: max(100 x the 2.374e-12 measured there, 1e-9) = 1e-9."""
import functools

import numpy as np
import pytest

import _front_scene as S
import _match_ref as MR
import fivepoint_ref as F
from spherical_sfm_amd import _lib, match, pairwise, ransac

pytestmark = pytest.mark.gpu
THR = (2.0 / S.FOCAL) ** 2
MIN = 10
TOL = max(100.0 * 2.374e-12, 1e-9)
SIZES = (300, 130, 70, 300, 130, 70, 3, 2, 1, 0)


def compose(ctx, fp, descs, rays, pairs, ro, ratio=0.75):
    """the four steps of include/ssfm.h through match.py and ransac.py"""
    pr = np.asarray(pairs, np.int32).reshape(-1, 2)
    mp, m0, m1 = match.match_flat(ctx, fp, descs, pr[:, 0], pr[:, 1], ratio=ratio)
    cnt = np.diff(mp)
    cand = np.nonzero((cnt >= ro.min_num_inliers) & (cnt > 0))[0]
    out = dict(match_count=cnt.astype(np.int32), num_inliers_all=np.full(len(pr), -1, np.int32), iterations=np.zeros(len(pr), np.uint32), lo_runs=np.zeros(len(pr), np.uint32),
               accepted_pair=np.zeros(0, np.int32), R=np.zeros((0, 3, 3)), t=np.zeros((0, 3)), E=np.zeros((0, 3, 3)), num_inliers=np.zeros(0, np.int32),
               inl_ptr=np.zeros(1, np.int32), inl_idx0=np.zeros(0, np.int32), inl_idx1=np.zeros(0, np.int32))
    if len(cand) == 0:
        return out
    cp = np.zeros(len(cand) + 1, np.int32); cp[1:] = np.cumsum(cnt[cand])
    c0 = np.concatenate([m0[mp[p]:mp[p + 1]] for p in cand]); c1 = np.concatenate([m1[mp[p]:mp[p + 1]] for p in cand])
    r = ransac.ransac5_batch_indexed(ctx, fp, rays, pr[cand, 0], pr[cand, 1], cp, c0, c1, THR, options=ro)
    out["num_inliers_all"][cand] = r["num_inliers"]; out["iterations"][cand] = r["iterations"]; out["lo_runs"][cand] = r["lo_runs"]
    acc = [k for k in range(len(cand)) if r["num_inliers"][k] > ro.min_num_inliers and r["mask"][cp[k]:cp[k + 1]].any()]
    i0 = [c0[cp[k]:cp[k + 1]][r["mask"][cp[k]:cp[k + 1]] != 0] for k in acc]; i1 = [c1[cp[k]:cp[k + 1]][r["mask"][cp[k]:cp[k + 1]] != 0] for k in acc]
    ptr = np.zeros(len(acc) + 1, np.int32); ptr[1:] = np.cumsum([len(x) for x in i0])
    out.update(accepted_pair=cand[acc].astype(np.int32), R=r["R"][acc], t=r["t"][acc], E=r["E"][acc], num_inliers=r["num_inliers"][acc], inl_ptr=ptr,
               inl_idx0=np.concatenate(i0) if acc else np.zeros(0, np.int32), inl_idx1=np.concatenate(i1) if acc else np.zeros(0, np.int32))
    return out


KEYS = ("accepted_pair", "R", "t", "E", "num_inliers", "inl_ptr", "inl_idx0", "inl_idx1", "match_count", "num_inliers_all", "iterations", "lo_runs")


def same(res, ref, keys=KEYS):
    get = (lambda k: ref[k]) if isinstance(ref, dict) else (lambda k: getattr(ref, k))
    for k in keys:
        a, b = getattr(res, k), get(k)
        assert a.shape == b.shape and np.array_equal(a, b), (k, a, b)
    assert np.all(np.diff(res.accepted_pair) > 0)


def front(ctx, scene, ro, **kw):
    fp, descs, rays, pairs = scene
    return pairwise.pairwise5_from_features(ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR, **kw)


def make_scene(frames):
    fp, descs, rays = S.flatten(frames)
    return fp, descs, rays, match.exhaustive_pairs(len(frames))


@functools.lru_cache(maxsize=None)
def scene_of_dim(dim):
    return make_scene(S.arc_frames(SIZES, dim=dim, seed=dim))


@pytest.mark.parametrize("dim", [128, 8])
def test_every_output_equals_the_composition(gpu_ctx, dim):
    scene = scene_of_dim(dim)
    ro = ransac.default_options(min_num_inliers=MIN)
    ref = compose(gpu_ctx, *scene, ro)
    res = front(gpu_ctx, scene, ro)
    same(res, ref)
    assert len(res.accepted_pair) >= 5 and (res.match_count == 0).any() and (res.num_inliers_all == -1).any()
    assert np.all(np.diff(res.accepted_pair) > 0)
    assert pairwise.last_kernel_ms(gpu_ctx) > 0.0
    noE = front(gpu_ctx, scene, ro, want_E=False)                         # E = NULL: every other field is unchanged
    assert noE.E is None
    same(noE, ref, [k for k in KEYS if k != "E"])


def test_lists_equal_the_numpy_matcher_and_the_five_point_replay(gpu_ctx):
    """Independent of the library's own matching and estimator: match lists from tests/_match_ref.py, per candidate the replay of tests/fivepoint_ref.py.  Chosen
    on the CPU: 5 candidates with 21, 40, 26, 25 and 27 matches; the replay flags none as marginal and accepts all five (17, 31, 20, 19 and 23 inliers);
    pair (1, 3) has 7 matches and is no candidate.  At most one candidate may be left out as marginal."""
    frames = S.arc_frames((130, 70, 130, 70, 2), dim=128, seed=21)
    scene = make_scene(frames); fp, descs, rays, pairs = scene
    res = front(gpu_ctx, scene, ransac.default_options(min_num_inliers=MIN))
    mp, m0, m1 = MR.match_pairs([f[1] for f in frames], pairs)
    assert np.array_equal(res.match_count, np.diff(mp))
    assert [int(c) for c in np.diff(mp) if c >= MIN] == [21, 40, 26, 25, 27] and res.match_count[pairs.index((1, 3))] == 7
    marginal = 0; checked = 0
    for p, (a, b) in enumerate(pairs):
        n = mp[p + 1] - mp[p]
        if n < MIN or n == 0:
            assert res.num_inliers_all[p] == -1 and p not in res.accepted_pair
            continue
        j, i = m0[mp[p]:mp[p + 1]], m1[mp[p]:mp[p + 1]]
        rep = F.replay(rays[fp[a] + j], rays[fp[b] + i], THR, min_num_inliers=MIN)
        if rep["marginal"]:
            marginal += 1
            continue
        checked += 1
        assert res.iterations[p] == rep["iterations"] and res.lo_runs[p] == rep["lo_runs"] and res.num_inliers_all[p] == rep["num_inliers"], (p, rep["iterations"], rep["num_inliers"])
        assert (p in res.accepted_pair) == bool(rep["accepted"] and rep["mask"].any())
        if p in res.accepted_pair:
            k = int(np.nonzero(res.accepted_pair == p)[0][0]); g0, g1 = res.matches(k)
            assert res.num_inliers[k] == rep["num_inliers"]
            assert np.array_equal(g0, j[rep["mask"]]) and np.array_equal(g1, i[rep["mask"]])
            dE, dR, dt = F.sign_distance(res.E[k], rep["E"]), np.abs(res.R[k] - rep["R"]).max(), np.abs(res.t[k] - rep["t"]).max()
            print("pair", p, "E", dE, "R", dR, "t", dt)
            assert dE <= TOL and dR <= TOL and dt <= TOL, (p, dE, dR, dt)
    assert marginal <= 1 and checked >= 4, (marginal, checked)


def test_smallest_samples(gpu_ctx):
    """frame 0 holds points 0..39; frames 1..5 share exactly 4, 5, 6, 7 and 8 of them (disjoint blocks) plus 30 points of their own: pairs (0, k) have exactly
    that many matches and every other pair none.  Fewer than five correspondences give no model; n = 5..8 exact correspondences are all inliers (the replay
    says so; it calls these pairs marginal, so which E wins is not compared with it)."""
    counts = (4, 5, 6, 7, 8); start = np.concatenate([[0], np.cumsum(counts)])
    shared = {0: np.arange(0, 40)}
    for k, c in enumerate(counts):
        shared[k + 1] = np.concatenate([np.arange(start[k], start[k] + c), np.arange(40 + 30 * k, 70 + 30 * k)])
    frames = S.arc_frames((40, 34, 35, 36, 37, 38), dim=128, seed=41, shared=shared)
    scene = make_scene(frames); fp, descs, rays, pairs = scene
    ro = ransac.default_options(min_num_inliers=4)
    ref = compose(gpu_ctx, *scene, ro)
    res = front(gpu_ctx, scene, ro)
    same(res, ref)
    for p, (a, b) in enumerate(pairs):
        assert res.match_count[p] == (counts[b - 1] if a == 0 else 0), (a, b, res.match_count[p])
    p01 = pairs.index((0, 1))
    assert res.num_inliers_all[p01] == 0 and res.iterations[p01] == 0 and p01 not in res.accepted_pair      # a candidate (4 >= 4) without a model
    mp, m0, m1 = MR.match_pairs([f[1] for f in frames], pairs)
    for b in (2, 3, 4, 5):
        p = pairs.index((0, b)); n = counts[b - 1]
        assert p in res.accepted_pair
        k = int(np.nonzero(res.accepted_pair == p)[0][0]); g0, g1 = res.matches(k)
        j, i = m0[mp[p]:mp[p + 1]], m1[mp[p]:mp[p + 1]]
        rep = F.replay(rays[fp[0] + j], rays[fp[b] + i], THR, min_num_inliers=4)
        assert len(j) == n and rep["num_inliers"] == n and rep["mask"].all()
        assert res.num_inliers[k] == n and np.array_equal(g0, j) and np.array_equal(g1, i)
    ro8 = ransac.default_options(min_num_inliers=8)
    res8 = front(gpu_ctx, scene, ro8)
    same(res8, compose(gpu_ctx, *scene, ro8))
    p05 = pairs.index((0, 5))
    assert res8.num_inliers_all[p05] == 8 and p05 not in res8.accepted_pair and len(res8.accepted_pair) == 0           # num_inliers == min_num_inliers: rejected
    assert (np.delete(res8.num_inliers_all, p05) == -1).all()


def test_more_than_one_scan_chunk_per_pair(gpu_ctx):
    """pair (0, 1) has 360 matches, all inliers: its accepted list crosses the 256-entry chunks of the compaction scan"""
    scene = make_scene(S.arc_frames((400, 400, 60), dim=128, seed=43, wrong_frac=0.0, unrelated_frac=0.05, pool=400))
    ro = ransac.default_options(min_num_inliers=MIN)
    res = front(gpu_ctx, scene, ro)
    same(res, compose(gpu_ctx, *scene, ro))
    p = scene[3].index((0, 1))
    assert p in res.accepted_pair
    g0, g1 = res.matches(int(np.nonzero(res.accepted_pair == p)[0][0]))
    assert len(g0) > 256 and np.all(np.diff(g0) > 0)


def test_slabs_and_ray_placement_do_not_change_a_bit(gpu_ctx, monkeypatch):
    scene = scene_of_dim(128)
    ro = ransac.default_options(min_num_inliers=MIN)
    base = front(gpu_ctx, scene, ro)
    for env in ({"SSFM_MATCH_SLAB_PAIRS": "1"}, {"SSFM_MATCH_SLAB_PAIRS": "3"}, {"SSFM_RANSAC_SLAB_PAIRS": "4"}, {"SSFM_MATCH_SLAB_PAIRS": "7", "SSFM_RANSAC_SLAB_PAIRS": "1"},
                {"SSFM_RANSAC5_FORCE_GLOBAL": "1"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            res = front(gpu_ctx, scene, ro)
        same(res, base)


def test_capacity_protocol_and_empty_inputs(gpu_ctx):
    scene = scene_of_dim(128); fp, descs, rays, pairs = scene
    pr = np.asarray(pairs, np.int32); f0 = np.ascontiguousarray(pr[:, 0]); f1 = np.ascontiguousarray(pr[:, 1])
    mo = match.default_options(dim=descs.shape[1]); ro = ransac.default_options(min_num_inliers=MIN)
    full = front(gpu_ctx, scene, ro, pair_capacity=len(pairs), inlier_capacity=10 ** 6)
    A, T = len(full.accepted_pair), len(full.inl_idx0)
    assert full.calls == 1 and A > 3 and T > 100
    for pc, ic in ((A - 1, T), (A, T - 1), (0, 0)):
        out = pairwise.pairwise5_from_features_raw(gpu_ctx, fp, descs, rays, f0, f1, mo, ro, THR, pc, ic)
        assert out[0] == -1 and out[1].tolist() == [A, T]                                   # SSFM_ERR_INVALID, both sizes
        assert b"capacity" in _lib.lib().ssfm_last_error(gpu_ctx._p)
    out = pairwise.pairwise5_from_features_raw(gpu_ctx, fp, descs, rays, f0, f1, mo, ro, THR, A, T)      # exactly enough
    assert out[0] == 0 and np.array_equal(out[2][:A], full.accepted_pair) and np.array_equal(out[6][:T], full.inl_idx0)
    assert np.array_equal(out[11][:3 * A].reshape(A, 3), full.t)
    small = front(gpu_ctx, scene, ro, pair_capacity=1, inlier_capacity=1)
    assert small.calls == 2
    same(small, full)
    none = pairwise.pairwise5_from_features(gpu_ctx, descs, rays, fp, np.zeros((0, 2), np.int32), ransac_options=ro, sq_thresh=THR)
    assert len(none.accepted_pair) == 0 and none.inl_ptr.tolist() == [0] and len(none.match_count) == 0 and none.t.shape == (0, 3) and none.E.shape == (0, 3, 3)
    zero = pairwise.pairwise5_from_features(gpu_ctx, np.zeros((0, 128), np.float32), np.zeros((0, 3)), np.zeros(1, np.int32), np.zeros((0, 2), np.int32), sq_thresh=THR)
    assert len(zero.accepted_pair) == 0 and zero.inl_ptr.tolist() == [0]


def test_five_calls_give_the_same_bits(gpu_ctx):
    scene = scene_of_dim(128)
    ro = ransac.default_options(min_num_inliers=MIN)
    runs = [front(gpu_ctx, scene, ro) for _ in range(5)]
    for r in runs[1:]:
        same(r, runs[0])


def test_a_context_with_a_communicator_is_refused(gpu_ctx):
    """(needs a context, hence a device: the other argument checks are in tests/test_pairwise5_front_cpu.py)"""
    from spherical_sfm_amd import ba
    fp, descs, rays, pairs = scene_of_dim(128)
    ctx = ba.Context(0)
    try:
        hook = _lib.HOST_ALLREDUCE_FN(lambda user, buf, n, op: 0)
        _lib.check(_lib.lib().ssfm_comm_init_host(ctx._p, 1, 0, hook, None), ctx._p)
        with pytest.raises(_lib.SsfmError, match="ssfm_pairwise5_from_features.*communicator"):
            pairwise.pairwise5_from_features(ctx, descs, rays, fp, pairs, sq_thresh=THR)
    finally:
        ctx.close()


def test_the_spherical_call_is_untouched(gpu_ctx):
    fp, descs, rays, pairs = scene = scene_of_dim(128)
    ro = ransac.default_options(min_num_inliers=MIN)
    sph = lambda: pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR)
    before = sph()
    five = front(gpu_ctx, scene, ro)
    after = sph()
    assert len(before.accepted_pair) >= 5 and len(five.accepted_pair) >= 5
    same(after, before, [k for k in KEYS if k not in ("t", "E")])
