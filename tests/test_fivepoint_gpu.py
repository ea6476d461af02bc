"""General relative pose on the device (ssfm_ransac5_batch and its probes) against the numpy restatement tests/fivepoint_ref.py.
The restatement's replays are computed once per session and shared."""
import functools

import numpy as np
import pytest

import fivepoint_ref as F
from spherical_sfm_amd import ransac, synth

pytestmark = pytest.mark.gpu

FOCAL = 1000.0
THR = (2.0 / FOCAL) ** 2            # 2 px at f = 1000, squared, in normalised image coordinates
# Largest Frobenius distance (up to sign) between a device solution and the restatement's over the stable samples of the solver-probe test,
# measured once on an MI355X: see test_solver_probe (the figure is printed by the test and recorded in DESIGN.md section 4, "General relative pose").
SOLVER_MEASURED = 2.374e-12         # 100 x that is 2.4e-10: the floor of 1e-9 holds
SOLVER_TOL = 1e-9 if SOLVER_MEASURED is None else max(100.0 * SOLVER_MEASURED, 1e-9)
TRACE_SEED0 = 0                     # seeds TRACE_SEED0 + k of the 32 trace pairs; chosen on the CPU: the replay flags none of them as marginal
SOLVER_SEED = 7                     # with this seed the restatement leaves out 0 of the 256 probe samples (cap: 12 = 5 %)


def _rot_err_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0))))


def _flat(pairs):
    ptr = np.zeros(len(pairs) + 1, np.int32)
    for i, (u, _) in enumerate(pairs): ptr[i + 1] = ptr[i] + len(u)
    U = np.concatenate([np.asarray(u, float).reshape(-1, 3) for u, _ in pairs] + [np.zeros((0, 3))])
    V = np.concatenate([np.asarray(v, float).reshape(-1, 3) for _, v in pairs] + [np.zeros((0, 3))])
    return ptr, np.ascontiguousarray(U), np.ascontiguousarray(V)


@functools.lru_cache(maxsize=None)
def trace_pairs():
    """32 general-motion pairs of 60..400 correspondences, 30 % outliers, 0.5 px noise, with the replay of each"""
    rng = np.random.default_rng(TRACE_SEED0)
    sizes = rng.integers(60, 401, 32)
    probs = [synth.make_general_pose_problem(int(n), noise_px=0.5, outlier_frac=0.3, focal=FOCAL, seed=TRACE_SEED0 + k) for k, n in enumerate(sizes)]
    reps = [F.replay(p[0], p[1], THR) for p in probs]
    return probs, reps


def _check_against_replay(out, k, ptr, rep, tol):
    """pair k of a device result against its replay: stats, inlier count and mask exactly, E up to sign and R to tol"""
    assert out["iterations"][k] == rep["iterations"] and out["lo_runs"][k] == rep["lo_runs"], (k, out["iterations"][k], rep["iterations"], out["lo_runs"][k], rep["lo_runs"])
    assert out["num_inliers"][k] == rep["num_inliers"], (k, out["num_inliers"][k], rep["num_inliers"])
    assert np.array_equal(out["mask"][ptr[k]:ptr[k + 1]].astype(bool), rep["mask"]), k
    assert F.sign_distance(out["E"][k], rep["E"]) <= tol, (k, F.sign_distance(out["E"][k], rep["E"]))
    assert np.abs(out["R"][k] - rep["R"]).max() <= tol and np.abs(out["t"][k] - rep["t"]).max() <= tol, (k, np.abs(out["R"][k] - rep["R"]).max())


def _check_self_consistent(out, k, ptr, pair):
    """what holds for a pair whose replay is marginal (pairs of 5..9 noise-only correspondences draw the same few samples again and again, so equal fits
    compete on rounding noise): the mask is the residual of the returned E below the threshold, E is an essential matrix through five of the rays, R a rotation"""
    u, v = pair; E = out["E"][k]; mask = out["mask"][ptr[k]:ptr[k + 1]].astype(bool)
    r = F.residual(E, u, v)
    sure = np.abs(r - THR) > 1e-9 * THR
    assert np.array_equal(mask[sure], (r < THR)[sure]) and mask.sum() == out["num_inliers"][k]
    assert abs(np.linalg.norm(E) - 1) <= 1e-12 and abs(np.linalg.det(E)) <= 1e-9 and np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max() <= 1e-9
    assert np.sort(np.abs(np.einsum("ni,ij,nj->n", v, E, u)))[4] <= 1e-9
    R = out["R"][k]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12 and abs(np.linalg.norm(out["t"][k]) - 1) <= 1e-12


# ---- 1. the minimal solver -----------------------------------------------------------------------------------------------------------
def test_solver_probe(gpu_ctx):
    rng = np.random.default_rng(SOLVER_SEED)
    us, vs, samples = [], [], []
    for k in range(4):                                       # 4 pairs of 40 rays: two noise-free, two with 0.5 px noise; 64 samples each
        u, v, *_ = synth.make_general_pose_problem(40, noise_px=0.0 if k < 2 else 0.5, focal=FOCAL, seed=SOLVER_SEED * 10 + k)
        us.append(u); vs.append(v)
        samples += [40 * k + rng.choice(40, 5, replace=False) for _ in range(64)]
    # degenerate samples: five identical rays, five coplanar points
    ident = np.tile([[0.1, -0.2, 1.0]], (5, 1))
    X = np.c_[rng.uniform(-1, 1, (5, 2)), np.full(5, 5.0)]; Rr = synth.so3exp(np.array([0.1, -0.2, 0.05])); P2 = X @ Rr.T + np.array([0.3, 0.1, -0.2])
    us += [ident, X / X[:, 2:]]; vs += [ident, P2 / P2[:, 2:]]
    samples += [160 + np.arange(5), 165 + np.arange(5)]
    U = np.concatenate(us); V = np.concatenate(vs); S = np.array(samples, np.int32)
    got = ransac.fivepoint_solver_probe(gpu_ctx, U, V, S)
    assert len(got) == 258
    for Es in got:
        assert np.isfinite(np.array(Es)).all() if len(Es) else True
        for E in Es: assert abs(np.linalg.norm(E) - 1.0) <= 1e-12
    assert len(got[256]) == 0                                # rank-deficient: no model
    left_out, worst = 0, 0.0
    for s in range(256):
        ref, _, w, _ = F.solve_full(U[S[s]], V[S[s]])
        if F.sample_is_unstable(ref, w): left_out += 1; continue
        assert len(got[s]) == len(ref), (s, len(got[s]), len(ref))
        for E in ref: worst = max(worst, min(F.sign_distance(E, G) for G in got[s]))
        for G in got[s]: worst = max(worst, min(F.sign_distance(E, G) for E in ref))
    print(f"solver probe: largest distance device <-> restatement {worst:.3e}, left out {left_out} of 256")
    assert left_out <= 12                                    # 5 %; SOLVER_SEED leaves out 0
    assert worst <= SOLVER_TOL, worst


# ---- 2. the residual --------------------------------------------------------------------------------------------------------------
def test_residual_probe(gpu_ctx):
    # 10 models x 257 rays (a partial last wave).  d = v . E (u / u2) cancels: its relative error is that of the sum's terms times
    # cond = sum |terms| / |d|, and the residual squares it.  The seed is chosen (on the CPU) so that cond <= 500 on all 2570 entries:
    # 2 * 500 * (3 roundings of 1.1e-16) = 3.3e-13 < 1e-12.  The comparison value is computed in extended precision.
    rng = np.random.default_rng(4)                           # seed 4: largest cond 484
    Es = rng.normal(size=(10, 3, 3)); Es /= np.linalg.norm(Es, axis=(1, 2), keepdims=True)
    u = np.c_[rng.uniform(-0.8, 0.8, (257, 2)), rng.uniform(0.5, 2.0, 257)]; v = np.c_[rng.uniform(-0.8, 0.8, (257, 2)), rng.uniform(0.5, 2.0, 257)]
    ld = np.longdouble
    line = np.einsum("tij,nj->tni", Es.astype(ld), (u / u[:, 2:]).astype(ld))
    terms = line * v.astype(ld)[None]
    d = terms.sum(-1)
    cond = np.abs(terms).sum(-1) / np.abs(d)
    assert cond.max() <= 500, cond.max()
    want = (d * d / (line[..., 0] ** 2 + line[..., 1] ** 2)).astype(float)
    got = ransac.fivepoint_residual_probe(gpu_ctx, u, v, Es)
    rel = np.abs(got - want) / want
    print(f"residual probe: largest relative error {rel.max():.3e} (largest cond {float(cond.max()):.1f})")
    assert rel.max() <= 1e-12
    assert np.abs(F.residual(Es[3], u, v) - want[3]).max() <= 1e-11 * want[3].max()           # the restatement's own residual is the same function


# ---- 3. pose from E ------------------------------------------------------------------------------------------------------------------
def test_pose_probe(gpu_ctx):
    rng = np.random.default_rng(5)
    probs = [synth.make_general_pose_problem(300, noise_px=0.5, outlier_frac=0.2, focal=FOCAL, seed=50 + k) for k in range(8)]
    U = np.concatenate([p[0] for p in probs]); V = np.concatenate([p[1] for p in probs])
    sizes = [1, 5, 63, 64, 65, 300]
    lists, Es, owner = [], [], []
    for tsk in range(63):
        k = tsk % 8; m = sizes[tsk % 6]
        lists.append(300 * k + (np.arange(300) if m == 300 else rng.choice(300, m, replace=False)))
        Es.append(probs[k][4] / np.linalg.norm(probs[k][4])); owner.append(k)
    # a tie: one correspondence that all four candidates reject (found on the CPU), so every count is 0 and the last candidate wins
    E0 = Es[0]
    tie = next(q for q in range(300) if F.pose_from_E(E0, U, V, [q])[2].sum() == 0)          # (ray 35 of pair 0, an outlier)
    lists.append(np.array([tie])); Es.append(E0)
    R, t, votes = ransac.fivepoint_pose_probe(gpu_ctx, U, V, lists, Es)
    worst = 0.0
    for k in range(64):
        Rr, tr, vr = F.pose_from_E(Es[k], U, V, lists[k])
        assert np.array_equal(votes[k], vr), (k, votes[k], vr)
        worst = max(worst, np.abs(R[k] - Rr).max(), np.abs(t[k] - tr).max())
    assert worst <= 1e-9, worst
    R1, R2, t0 = F.decompose(Es[63])
    assert not votes[63].any() and np.abs(R[63] - R2).max() <= 1e-9 and np.abs(t[63] + t0).max() <= 1e-9      # (R2, -t): the last of four equal counts
    # the full lists of the true E recover the true pose
    for k in range(63):
        if len(lists[k]) == 300: assert _rot_err_deg(R[k], probs[owner[k]][2]) < 1e-6


# ---- 4. the trace ---------------------------------------------------------------------------------------------------------------------
def test_trace_equals_the_replay(gpu_ctx):
    probs, reps = trace_pairs()
    ptr, U, V = _flat([(p[0], p[1]) for p in probs])
    out = ransac.ransac5_batch(gpu_ctx, ptr, U, V, THR)
    flagged = [k for k, r in enumerate(reps) if r["marginal"]]
    print("trace: pairs the replay flags as marginal:", flagged)
    assert len(flagged) <= 2
    for k, rep in enumerate(reps):
        if k in flagged: continue
        _check_against_replay(out, k, ptr, rep, SOLVER_TOL)
        assert rep["accepted"] and _rot_err_deg(out["R"][k], probs[k][2]) < 2.0


# ---- 4b. the branches of the control flow that the default options hardly reach ------------------------------------------------------
# (lomsac_trace.h) the local optimisation at the first iteration, inside the first chunk, on a chunk boundary and never before the tail; chunks shorter
# than min_num_iterations_; a one-iteration second chunk; a fixed budget across three chunks; a budget that ends before lo_starting_iterations_
TRACE_OPTION_GRID = [dict(lo_start=0), dict(lo_start=1), dict(lo_start=127), dict(lo_start=128), dict(lo_start=100000), dict(min_it=1, lo_start=0),
                     dict(min_it=20, lo_start=50), dict(min_it=129), dict(min_it=300, max_it=300, lo_start=256), dict(min_it=10, max_it=10, lo_start=50)]
OPTION_FIELD = dict(min_it="min_num_iterations", max_it="max_num_iterations", lo_start="lo_starting_iterations")


@functools.lru_cache(maxsize=None)
def grid_pairs():
    """two pairs of 12 correspondences without outliers, two of 40 with 50 % outliers (377 and 496 iterations with the default options: three and four
    chunks, the later ones refill the sampler's FIFO), with the replay of each under every option set (about a second per replay)"""
    probs = [synth.make_general_pose_problem(n, noise_px=0.5, outlier_frac=frac, focal=FOCAL, seed=seed) for n, frac in ((12, 0.0), (40, 0.5)) for seed in (900, 901)]
    reps = [[F.replay(p[0], p[1], THR, **opts) for p in probs] for opts in TRACE_OPTION_GRID]
    return probs, reps


def test_rarely_taken_branches_of_the_control_flow(gpu_ctx):
    probs, reps = grid_pairs()
    ptr, U, V = _flat([(p[0], p[1]) for p in probs])
    for opts, rep4 in zip(TRACE_OPTION_GRID, reps):
        out = ransac.ransac5_batch(gpu_ctx, ptr, U, V, THR, **{OPTION_FIELD[k]: v for k, v in opts.items()})
        for k, rep in enumerate(rep4):
            print(opts, k, "iterations", out["iterations"][k], rep["iterations"], "lo runs", out["lo_runs"][k], rep["lo_runs"], "inliers", out["num_inliers"][k], rep["num_inliers"],
                  "E %.2e" % F.sign_distance(out["E"][k], rep["E"]))
            assert not rep["marginal"], (opts, k)                # chosen on the CPU: the replay flags none of the 40 cases
            _check_against_replay(out, k, ptr, rep, SOLVER_TOL)


# ---- 5. small and odd shapes, both ray placements ------------------------------------------------------------------------------------
def test_small_shapes_and_both_ray_placements(gpu_ctx, monkeypatch):
    big_n = ransac.fivepoint_max_lds_rays() + 1                # the first size whose rays stay in global memory, from the kernel's own layout
    sizes = [0, 4, 5, 6, 7, 8, 9, 128]
    # seeds chosen on the CPU so that the replay flags none of n = 6, 7, 8, 9, 128 as marginal (asserted below).  n = 5 is marginal by construction: every
    # candidate passes through all five rays, so equal fits compete on rounding noise
    seeds = {0: 300, 4: 304, 5: 305, 6: 20, 7: 4, 8: 308, 9: 3, 128: 428}
    probs = [synth.make_general_pose_problem(max(n, 1), noise_px=0.5, outlier_frac=0.25 if n >= 128 else 0.0, focal=FOCAL, seed=seeds[n]) for n in sizes]
    small = [(p[0][:n], p[1][:n]) for p, n in zip(probs, sizes)]
    bigp = synth.make_general_pose_problem(big_n, noise_px=0.5, outlier_frac=0.3, focal=FOCAL, seed=77)
    ptr, U, V = _flat(small)
    lds = ransac.ransac5_batch(gpu_ctx, ptr, U, V, THR)
    for k, n in enumerate(sizes):
        if n < 5:
            assert lds["num_inliers"][k] == 0 and lds["iterations"][k] == 0 and not lds["mask"][ptr[k]:ptr[k + 1]].any()
            assert np.array_equal(lds["R"][k], np.eye(3)) and not lds["t"][k].any() and not lds["E"][k].any()
            continue
        rep = F.replay(small[k][0], small[k][1], THR)
        if n == 5:
            # which of the equal-score candidates wins is rounding; the trace, the count and the mask do not depend on it
            assert rep["marginal"] and rep["num_inliers"] == 5 and rep["mask"].all()
            assert (lds["iterations"][k], lds["lo_runs"][k], lds["num_inliers"][k]) == (rep["iterations"], rep["lo_runs"], 5)
            assert lds["mask"][ptr[k]:ptr[k + 1]].all()
            _check_self_consistent(lds, k, ptr, small[k])
            continue
        assert not rep["marginal"], n
        _check_against_replay(lds, k, ptr, rep, SOLVER_TOL)      # n = 6, 7: ShuffleSample; n = 8: the first DrawSample size
    # the same pairs through the global-memory variant: forced by the switch, and beside a pair too large for LDS -- bit for bit
    monkeypatch.setenv("SSFM_RANSAC5_FORCE_GLOBAL", "1")
    forced = ransac.ransac5_batch(gpu_ctx, ptr, U, V, THR)
    monkeypatch.delenv("SSFM_RANSAC5_FORCE_GLOBAL")
    ptr2, U2, V2 = _flat(small + [(bigp[0], bigp[1])])
    mixed = ransac.ransac5_batch(gpu_ctx, ptr2, U2, V2, THR)
    for key in ("E", "R", "t", "num_inliers", "scores", "iterations", "lo_runs"):
        assert np.array_equal(lds[key], forced[key]), key
        assert np.array_equal(lds[key], mixed[key][:len(sizes)]), key
    assert np.array_equal(lds["mask"], forced["mask"]) and np.array_equal(lds["mask"], mixed["mask"][:ptr[-1]])
    rep = F.replay(bigp[0], bigp[1], THR)
    assert not rep["marginal"]
    _check_against_replay(mixed, len(sizes), ptr2, rep, SOLVER_TOL)


# ---- 6. what the feature is for ------------------------------------------------------------------------------------------------------
def test_general_motion_is_estimated_where_the_spherical_estimator_is_not(gpu_ctx):
    probs, reps = trace_pairs()
    probs, reps = probs[:16], reps[:16]
    ptr, U, V = _flat([(p[0], p[1]) for p in probs])
    five = ransac.ransac5_batch(gpu_ctx, ptr, U, V, THR, min_num_inliers=20)
    sph = ransac.estimate_flat(gpu_ctx, ptr, U, V, THR, min_num_inliers=20)
    acc5 = five["num_inliers"] > 20; accs = sph["num_inliers"] > 20
    # the bound: the replay's own largest rotation error on these pairs (the replay is the reference), times 2 for the cheirality vote near ties.
    # Measured on an MI355X: replay 0.4121 deg (bound 0.8242 deg), five-point 0.4121 deg, 16 of 16 accepted; the spherical estimator accepts 11 of 16 with a
    # median rotation error of 8.5 deg.
    ref_err = max(_rot_err_deg(r["R"], p[2]) for r, p in zip(reps, probs))
    err5 = [_rot_err_deg(five["R"][k], probs[k][2]) for k in range(16)]
    errs = [_rot_err_deg(sph["R"][k], probs[k][2]) for k in range(16)]
    print(f"five-point: accepted {acc5.sum()}/16, largest rotation error {max(err5):.4f} deg (replay {ref_err:.4f} deg); "
          f"spherical: accepted {accs.sum()}/16, median rotation error {np.median(errs):.3f} deg")
    assert acc5.all()
    assert max(err5) <= 2.0 * ref_err
    assert acc5.sum() >= accs.sum()


# ---- 7. indexed = materialised -----------------------------------------------------------------------------------------------------
def test_indexed_entry_point_equals_materialised_rays(gpu_ctx):
    rng = np.random.default_rng(8)
    frames = [[] for _ in range(8)]                          # per-frame feature rays
    pairs = [(a, b) for a in range(8) for b in range(a + 1, 8)][::2][:12]
    f0, f1, mptr, i0, i1, mats = [], [], [0], [], [], []
    for k, (a, b) in enumerate(pairs):
        n = int(rng.integers(30, 120))
        u, v, *_ = synth.make_general_pose_problem(n, noise_px=0.5, outlier_frac=0.2, focal=FOCAL, seed=600 + k)
        ia = len(frames[a]) + np.arange(n); ib = len(frames[b]) + np.arange(n)
        frames[a] += list(u); frames[b] += list(v)
        f0.append(a); f1.append(b); i0 += list(ia); i1 += list(ib); mptr.append(mptr[-1] + n); mats.append((u, v))
    feat_ptr = np.cumsum([0] + [len(f) for f in frames]).astype(np.int32)
    feat_rays = np.concatenate([np.array(f).reshape(-1, 3) for f in frames])
    idx = ransac.ransac5_batch_indexed(gpu_ctx, feat_ptr, feat_rays, f0, f1, mptr, i0, i1, THR, min_num_inliers=10)
    ptr, U, V = _flat(mats)
    mat = ransac.ransac5_batch(gpu_ctx, ptr, U, V, THR, min_num_inliers=10)
    for key in ("E", "R", "t", "mask", "num_inliers", "scores", "iterations", "lo_runs"):
        assert np.array_equal(idx[key], mat[key]), key
    assert (mat["num_inliers"] > 10).all()


# ---- 8. slabs, 9. repeatability ----------------------------------------------------------------------------------------------------
def test_slabs_and_repeatability(gpu_ctx, monkeypatch):
    probs = [synth.make_general_pose_problem(20, noise_px=0.5, outlier_frac=0.2, focal=FOCAL, seed=2000 + k) for k in range(300)]
    ptr, U, V = _flat([(p[0], p[1]) for p in probs])
    one = ransac.ransac5_batch(gpu_ctx, ptr, U, V, THR, min_num_inliers=8)
    again = ransac.ransac5_batch(gpu_ctx, ptr, U, V, THR, min_num_inliers=8)
    monkeypatch.setenv("SSFM_RANSAC_SLAB_PAIRS", "128")      # slabs of 128, 128, 44
    slabbed = ransac.ransac5_batch(gpu_ctx, ptr, U, V, THR, min_num_inliers=8)
    monkeypatch.delenv("SSFM_RANSAC_SLAB_PAIRS")
    for key in ("E", "R", "t", "mask", "num_inliers", "scores", "iterations", "lo_runs"):
        assert np.array_equal(one[key], again[key]), key
        assert np.array_equal(one[key], slabbed[key]), key
    assert (one["num_inliers"] > 8).sum() >= 250 and ransac.last_kernel_ms(gpu_ctx) > 0.0
