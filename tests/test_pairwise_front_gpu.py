"""ssfm_pairwise_from_features on the GPU: the call is DEFINED as the composition ssfm_match_pairs -> candidates -> ssfm_ransac_batch_indexed -> acceptance,
so every output is compared array_equal with that composition computed here from the two existing wrappers; one scene is also held against the numpy
matcher (tests/_match_ref.py) and the oracle's LO-MSAC."""
import os

import numpy as np
import pytest

import _front_scene as S
import _match_ref as MR
from spherical_sfm_amd import _lib, match, pairwise, ransac

pytestmark = pytest.mark.gpu
THR = (2.0 / S.FOCAL) ** 2
MIN = 10
SIZES = (300, 130, 70, 300, 130, 70, 3, 2, 1, 0)


def compose(ctx, fp, descs, rays, pairs, ro, ratio=0.75):
    """the four steps of include/ssfm.h through match.py and ransac.py"""
    pr = np.asarray(pairs, np.int32).reshape(-1, 2)
    mp, m0, m1 = match.match_flat(ctx, fp, descs, pr[:, 0], pr[:, 1], ratio=ratio)
    cnt = np.diff(mp)
    cand = np.nonzero((cnt >= ro.min_num_inliers) & (cnt > 0))[0]
    out = dict(match_count=cnt.astype(np.int32), num_inliers_all=np.full(len(pr), -1, np.int32), iterations=np.zeros(len(pr), np.uint32), lo_runs=np.zeros(len(pr), np.uint32),
               accepted_pair=np.zeros(0, np.int32), R=np.zeros((0, 3, 3)), num_inliers=np.zeros(0, np.int32), inl_ptr=np.zeros(1, np.int32),
               inl_idx0=np.zeros(0, np.int32), inl_idx1=np.zeros(0, np.int32), cand=cand, mp=mp, m0=m0, m1=m1)
    if len(cand) == 0:
        return out
    cp = np.zeros(len(cand) + 1, np.int32); cp[1:] = np.cumsum(cnt[cand])
    c0 = np.concatenate([m0[mp[p]:mp[p + 1]] for p in cand]); c1 = np.concatenate([m1[mp[p]:mp[p + 1]] for p in cand])
    r = ransac.estimate_indexed(ctx, fp, rays, pr[cand, 0], pr[cand, 1], cp, c0, c1, THR, options=ro)
    out["num_inliers_all"][cand] = r["num_inliers"]; out["iterations"][cand] = r["iterations"]; out["lo_runs"][cand] = r["lo_runs"]
    acc = [k for k in range(len(cand)) if r["num_inliers"][k] > ro.min_num_inliers and r["mask"][cp[k]:cp[k + 1]].any()]
    i0 = [c0[cp[k]:cp[k + 1]][r["mask"][cp[k]:cp[k + 1]] != 0] for k in acc]; i1 = [c1[cp[k]:cp[k + 1]][r["mask"][cp[k]:cp[k + 1]] != 0] for k in acc]
    ptr = np.zeros(len(acc) + 1, np.int32); ptr[1:] = np.cumsum([len(x) for x in i0])
    out.update(accepted_pair=cand[acc].astype(np.int32), R=r["R"][acc], num_inliers=r["num_inliers"][acc], inl_ptr=ptr, ransac=r, cand_ptr=cp,
               inl_idx0=np.concatenate(i0) if acc else np.zeros(0, np.int32), inl_idx1=np.concatenate(i1) if acc else np.zeros(0, np.int32))
    return out


KEYS = ("accepted_pair", "R", "num_inliers", "inl_ptr", "inl_idx0", "inl_idx1", "match_count", "num_inliers_all", "iterations", "lo_runs")


def same(res, ref):
    for k in KEYS:
        a, b = getattr(res, k), ref[k]
        assert a.shape == b.shape and np.array_equal(a, b), (k, a, b)
    assert np.all(np.diff(res.accepted_pair) > 0)


@pytest.fixture(scope="module", params=[128, 8])
def scene(request):
    fp, descs, rays = S.flatten(S.arc_frames(SIZES, dim=request.param, seed=request.param))
    return fp, descs, rays, match.exhaustive_pairs(len(SIZES))


@pytest.mark.parametrize("lsq,inward", [(1, 0), (0, 0), (1, 1), (0, 1)])
def test_every_output_equals_the_composition(gpu_ctx, scene, lsq, inward):
    fp, descs, rays, pairs = scene
    ro = ransac.default_options(min_num_inliers=MIN, final_least_squares=lsq, inward=inward)
    ref = compose(gpu_ctx, fp, descs, rays, pairs, ro)
    res = pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR)
    same(res, ref)
    assert len(res.accepted_pair) >= 5 and (ref["match_count"] == 0).any() and (res.num_inliers_all == -1).any()
    assert pairwise.last_kernel_ms(gpu_ctx) > 0.0
    if lsq == 1 and inward == 0:                                           # the fixed-budget mode draws per-pair streams: candidate k must get stream k
        ro = ransac.default_options(min_num_inliers=MIN, mode=ransac.RANSAC_FIXED_BUDGET, num_hypotheses=256, seed=5)
        same(pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR), compose(gpu_ctx, fp, descs, rays, pairs, ro))


def test_lists_equal_the_numpy_matcher_and_the_oracle_lomsac(gpu_ctx, oracle):
    """Independent of the library's own matching and RANSAC: match lists from tests/_match_ref.py, LO-MSAC from the oracle, with the identity rule and the
    1e-9 rotation tolerance of tests/test_ransac_trace_gpu.py (same iterations and LO runs, same inlier set, R to 1e-9, on >= 97 % of the pairs)."""
    frames = S.arc_frames((130, 70, 130, 70, 2), dim=128, seed=21)
    fp, descs, rays = S.flatten(frames); pairs = match.exhaustive_pairs(len(frames))
    ro = ransac.default_options(min_num_inliers=MIN)
    res = pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR)
    mp, m0, m1 = MR.match_pairs([f[1] for f in frames], pairs)
    assert np.array_equal(res.match_count, np.diff(mp))
    ok = []; expect = []
    for p, (a, b) in enumerate(pairs):
        n = mp[p + 1] - mp[p]
        if n < MIN or n == 0:
            assert res.num_inliers_all[p] == -1
            continue
        j, i = m0[mp[p]:mp[p + 1]], m1[mp[p]:mp[p + 1]]
        o = oracle.lomsac_pair(rays[fp[a] + j], rays[fp[b] + i], THR, min_num_inliers=MIN)
        inl = np.asarray(o["inliers"]).astype(bool)
        if not (inl.sum() > MIN):
            ok.append(p not in res.accepted_pair)
            continue
        expect.append(p)
        if p not in res.accepted_pair:
            ok.append(False)
            continue
        k = int(np.nonzero(res.accepted_pair == p)[0][0]); g0, g1 = res.matches(k)
        ok.append(res.iterations[p] == o["iterations"] and res.lo_runs[p] == o["lo_runs"] and np.array_equal(g0, j[inl]) and np.array_equal(g1, i[inl])
                  and np.abs(res.R[k] - o["R"]).max() <= 1e-9)
    assert len(expect) >= 3 and np.mean(ok) >= 0.97, ok


def test_filters_land_where_the_composition_puts_them(gpu_ctx):
    """frames 0 / 1 share exactly MIN - 1 points, frames 0 / 2 exactly MIN, frame 3 is unrelated to all; then min_num_inliers is set to the inlier count a
    candidate reaches, which the strict test of :410 rejects"""
    shared = {0: np.arange(0, 40), 1: np.concatenate([np.arange(0, MIN - 1), np.arange(100, 130)]), 2: np.concatenate([np.arange(30, 30 + MIN), np.arange(200, 240)]),
              4: np.arange(0, 35), 5: np.arange(5, 40)}
    frames = S.arc_frames((40, 39, 50, 40, 35, 35), dim=128, seed=33, shared=shared)
    frames[3] = S.arc_frames((40,), dim=128, seed=77)[0]                      # another world
    fp, descs, rays = S.flatten(frames); pairs = match.exhaustive_pairs(len(frames))
    ro = ransac.default_options(min_num_inliers=MIN)
    ref = compose(gpu_ctx, fp, descs, rays, pairs, ro)
    res = pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR)
    same(res, ref)
    p01, p02 = pairs.index((0, 1)), pairs.index((0, 2))
    assert res.match_count[p01] == MIN - 1 and res.num_inliers_all[p01] == -1 and p01 not in res.accepted_pair
    assert res.match_count[p02] == MIN and res.num_inliers_all[p02] >= 0                    # a candidate: >= is the rule of :353
    for p, (a, b) in enumerate(pairs):
        if 3 in (a, b):
            assert res.match_count[p] < MIN and p not in res.accepted_pair
    p45 = pairs.index((4, 5)); n45 = int(res.num_inliers_all[p45])
    assert p45 in res.accepted_pair and n45 > MIN
    ro2 = ransac.default_options(min_num_inliers=n45)
    ref2 = compose(gpu_ctx, fp, descs, rays, pairs, ro2)
    res2 = pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro2, sq_thresh=THR)
    same(res2, ref2)
    assert res2.num_inliers_all[p45] == n45 and p45 not in res2.accepted_pair               # num_inliers == min_num_inliers: rejected


def test_slabs_do_not_change_the_output(gpu_ctx, scene, monkeypatch):
    fp, descs, rays, pairs = scene
    ro = ransac.default_options(min_num_inliers=MIN)
    base = pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR)
    for env in ({"SSFM_MATCH_SLAB_PAIRS": "1"}, {"SSFM_MATCH_SLAB_PAIRS": "3"}, {"SSFM_RANSAC_SLAB_PAIRS": "4"}, {"SSFM_MATCH_SLAB_PAIRS": "7", "SSFM_RANSAC_SLAB_PAIRS": "1"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            res = pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR)
        same(res, {k: getattr(base, k) for k in KEYS})


def test_capacity_protocol_and_empty_inputs(gpu_ctx, scene):
    fp, descs, rays, pairs = scene
    pr = np.asarray(pairs, np.int32); f0 = np.ascontiguousarray(pr[:, 0]); f1 = np.ascontiguousarray(pr[:, 1])
    mo = match.default_options(dim=descs.shape[1]); ro = ransac.default_options(min_num_inliers=MIN)
    full = pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR, pair_capacity=len(pairs), inlier_capacity=10 ** 6)
    A, T = len(full.accepted_pair), len(full.inl_idx0)
    assert full.calls == 1 and A > 3 and T > 100
    for pc, ic in ((A - 1, T), (A, T - 1), (0, 0), (1, 10 ** 6)):
        out = pairwise.pairwise_from_features_raw(gpu_ctx, fp, descs, rays, f0, f1, mo, ro, THR, pc, ic)
        assert out[0] == -1 and out[1].tolist() == [A, T]                                   # SSFM_ERR_INVALID, both sizes
        assert b"capacity" in _lib.lib().ssfm_last_error(gpu_ctx._p)
    out = pairwise.pairwise_from_features_raw(gpu_ctx, fp, descs, rays, f0, f1, mo, ro, THR, A, T)      # exactly enough
    assert out[0] == 0 and np.array_equal(out[2][:A], full.accepted_pair) and np.array_equal(out[6][:T], full.inl_idx0)
    small = pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR, pair_capacity=1, inlier_capacity=1)
    assert small.calls == 2
    same(small, {k: getattr(full, k) for k in KEYS})
    none = pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, np.zeros((0, 2), np.int32), ransac_options=ro, sq_thresh=THR)
    assert len(none.accepted_pair) == 0 and none.inl_ptr.tolist() == [0] and len(none.match_count) == 0
    zero = pairwise.pairwise_from_features(gpu_ctx, np.zeros((0, 128), np.float32), np.zeros((0, 3)), np.zeros(1, np.int32), np.zeros((0, 2), np.int32), sq_thresh=THR)
    assert len(zero.accepted_pair) == 0 and zero.inl_ptr.tolist() == [0]


def test_five_calls_give_the_same_bits(gpu_ctx, scene):
    fp, descs, rays, pairs = scene
    ro = ransac.default_options(min_num_inliers=MIN)
    runs = [pairwise.pairwise_from_features(gpu_ctx, descs, rays, fp, pairs, ransac_options=ro, sq_thresh=THR) for _ in range(5)]
    for r in runs[1:]:
        same(r, {k: getattr(runs[0], k) for k in KEYS})


def test_a_context_with_a_communicator_is_refused(gpu_ctx, scene):
    """(needs a context, hence a device: the other argument checks are in tests/test_pairwise_front_cpu.py)"""
    from spherical_sfm_amd import ba
    fp, descs, rays, pairs = scene
    ctx = ba.Context(0)
    try:
        hook = _lib.HOST_ALLREDUCE_FN(lambda user, buf, n, op: 0)
        _lib.check(_lib.lib().ssfm_comm_init_host(ctx._p, 1, 0, hook, None), ctx._p)
        with pytest.raises(_lib.SsfmError, match="communicator"):
            pairwise.pairwise_from_features(ctx, descs, rays, fp, pairs, sq_thresh=THR)
    finally:
        ctx.close()
