"""Test-only restatement of ssfm_rot_l1_init (include/ssfm.h) in numpy, and the fixtures tests/test_rot_l1_cpu.py and tests/test_rot_l1_gpu.py share.

* l1_irls(..., solver="dense"): the algorithm of the header with numpy.linalg.solve on the reduced Laplacian -- the primary restatement.
* l1_irls(..., solver="pcg"): the same outer loop with Jacobi-preconditioned conjugate gradients under the header's stopping rule (three columns in lockstep, the
  test before each iteration, the cap), for the capped case and for the floor under the parity tolerance.
* fixtures: shuffled rings with gross outliers, a complete graph with a corrupted tree edge, a pure chain, two components; _view_graph_ref.edge_cases() as it is."""
import functools

import numpy as np

from spherical_sfm_amd import synth

import _view_graph_ref as VR

DEFAULTS = dict(max_iterations=30, step_tolerance=1e-4, weight_floor=1e-3, pcg_tolerance=1e-10, pcg_max_iterations=0)
CONVERGENCE, NO_CONVERGENCE = 0, 1
CUT = np.deg2rad(2.0)


def so3ln(R):
    """(...,3,3) -> (...,3): the log map by atan2(|sin part|, cos part); exact enough below pi - 1e-6, which every residual of the fixtures is"""
    s = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)
    sn = np.linalg.norm(s, axis=-1)
    ang = np.arctan2(sn, c)
    k = np.where(sn > 0, ang / np.where(sn > 0, sn, 1.0), 1.0)
    return s * k[..., None]


def geodesic(Ra, Rb):
    """angle of Ra Rb^T per camera, radians"""
    return np.linalg.norm(so3ln(Ra @ np.transpose(Rb, (0, 2, 1))), axis=-1)


def error_to_truth_deg(R, R_gt, root):
    """per-camera error against the ground truth in the gauge of the result (R_root = I)"""
    return np.rad2deg(geodesic(R, R_gt @ R_gt[root].T))


def _pcg(L, d, g, tol, cap):
    """three columns in lockstep -> x, lockstep iterations, capped"""
    m = len(d)
    x = np.zeros((m, 3)); r = g.copy(); z = r / d[:, None]; p = z.copy()
    rz = (r * z).sum(0); gg = (g * g).sum(0); rr = gg.copy()
    done = rr <= tol * tol * gg
    it = 0
    while not done.all():
        if it >= cap:
            return x, it, True
        act = ~done
        q = L @ p
        alpha = np.where(act, rz / np.where(act, (p * q).sum(0), 1.0), 0.0)
        x += alpha * p; r -= alpha * q
        z = r / d[:, None]
        rz_new = (r * z).sum(0); rr = (r * r).sum(0)
        beta = np.where(act, rz_new / np.where(act, rz, 1.0), 0.0)
        p = np.where(act, z + beta * p, p)
        rz = np.where(act, rz_new, rz)
        done = done | (act & (rr <= tol * tol * gg))
        it += 1
    return x, it, False


def l1_irls(n, i0, i1, rel, root=0, solver="dense", **options):
    """-> rotations (n,3,3), residuals (E,), summary dict (the keys of ssfm_rot_l1_summary without kernel_ms)"""
    o = dict(DEFAULTS); o.update(options)
    i0 = np.asarray(i0); i1 = np.asarray(i1); rel = np.asarray(rel, np.float64); E = len(i0)
    tree = VR.bfs_tree(n, i0, i1, root)
    R = VR.chain_tree(n, tree, rel)
    reached = np.zeros(n, bool); reached[tree["node"][:tree["num_reached"]]] = True
    used = (i0 != i1) & reached[i0] & reached[i1] if E else np.zeros(0, bool)
    free = reached.copy(); free[root] = False
    idx = -np.ones(n, np.int64); idx[free] = np.arange(free.sum()); m = int(free.sum())
    a, b = i0[used], i1[used]
    s = dict(iterations=0, termination=CONVERGENCE, num_free=m, num_edges_used=int(used.sum()), pcg_solves_capped=0, pcg_iterations_total=0, initial_cost=0.0,
             final_cost=0.0, last_step=0.0)
    res = -np.ones(E)
    if not used.any():
        return R, res, s

    def residuals():
        return so3ln(np.transpose(R[b], (0, 2, 1)) @ rel[used] @ R[a])

    cap = o["pcg_max_iterations"] or 4 * m
    for k in range(1, o["max_iterations"] + 1):
        v = residuals(); nv = np.linalg.norm(v, axis=1)
        if k == 1:
            s["initial_cost"] = float(nv.sum())
        w = 1.0 / np.maximum(nv, o["weight_floor"])
        L = np.zeros((m, m)); g = np.zeros((m, 3))
        ia, ib = idx[a], idx[b]
        fa, fb = ia >= 0, ib >= 0
        np.add.at(L, (ia[fa], ia[fa]), w[fa]); np.add.at(L, (ib[fb], ib[fb]), w[fb])
        both = fa & fb
        np.add.at(L, (ia[both], ib[both]), -w[both]); np.add.at(L, (ib[both], ia[both]), -w[both])
        np.add.at(g, ib[fb], (w[:, None] * v)[fb]); np.add.at(g, ia[fa], -(w[:, None] * v)[fa])
        if solver == "dense":
            x = np.linalg.solve(L, g)
        else:
            x, it, capped = _pcg(L, np.diag(L).copy(), g, o["pcg_tolerance"], cap)
            s["pcg_iterations_total"] += it; s["pcg_solves_capped"] += int(capped)
        R[free] = R[free] @ synth.so3exp(x)
        step = float(np.linalg.norm(x, axis=1).max())
        s["iterations"] = k; s["last_step"] = step
        if step < o["step_tolerance"]:
            s["termination"] = CONVERGENCE
            break
        s["termination"] = NO_CONVERGENCE
    nv = np.linalg.norm(residuals(), axis=1)
    res[used] = nv; s["final_cost"] = float(nv.sum())
    return R, res, s


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------------------------

def _axis_kick(rng, lo_deg, hi_deg):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    return synth.so3exp((ax * np.deg2rad(rng.uniform(lo_deg, hi_deg)))[None])[0]


def _ring(n, seed, offsets=(1, 2, 3, 5, 9), noise_deg=0.2, outlier_frac=0.15):
    """Shuffled ring: edges (i, i + d mod n) for the offsets, half of them stored the other way round, list shuffled; every edge carries 0.2 degrees of noise,
    15 % of them a further rotation of 20-170 degrees about a random axis -> n, i0, i1, R (E,3,3), R_gt (n,3,3), corrupted (E,) bool"""
    rng = np.random.default_rng(seed)
    R_gt = synth.so3exp(rng.normal(size=(n, 3)) * 0.8)
    pairs = [(i, (i + d) % n) for d in offsets for i in range(n)]
    pairs = [(q, p) if rng.random() < 0.5 else (p, q) for p, q in pairs]
    pairs = [pairs[k] for k in rng.permutation(len(pairs))]
    i0, i1 = np.array(pairs, np.int32).T
    R = np.stack([synth.so3exp(rng.normal(0.0, np.deg2rad(noise_deg), (1, 3)))[0] @ R_gt[q] @ R_gt[p].T for p, q in pairs])
    bad = np.zeros(len(pairs), bool); bad[rng.choice(len(pairs), int(round(outlier_frac * len(pairs))), replace=False)] = True
    for e in np.flatnonzero(bad):
        R[e] = _axis_kick(rng, 20.0, 170.0) @ R[e]
    return n, np.ascontiguousarray(i0), np.ascontiguousarray(i1), R, R_gt, bad


@functools.lru_cache(maxsize=None)
def ring60(seed):
    """60 cameras, 300 edges, 45 corrupted"""
    return _ring(60, seed)


@functools.lru_cache(maxsize=None)
def ring350(seed=0):
    """350 cameras, 1750 edges: 3 n = 1050 vector entries, CG solves of a hundred iterations and more"""
    return _ring(350, seed)


@functools.lru_cache(maxsize=None)
def complete24(seed=7):
    """All 276 pairs of 24 cameras, 25 % outliers, and list position 0 = (0, 1) -- the first tree edge of root 0 -- rotated by 60 degrees
    -> n, i0, i1, R, R_gt, corrupted"""
    rng = np.random.default_rng(seed); n = 24
    R_gt = synth.so3exp(rng.normal(size=(n, 3)) * 0.8)
    i0, i1 = np.array([(p, q) for p in range(n) for q in range(p + 1, n)], np.int32).T
    R = np.stack([synth.so3exp(rng.normal(0.0, np.deg2rad(0.2), (1, 3)))[0] @ R_gt[q] @ R_gt[p].T for p, q in zip(i0, i1)])
    bad = np.zeros(len(i0), bool); bad[rng.choice(np.arange(1, len(i0)), int(round(0.25 * len(i0))) - 1, replace=False)] = True
    for e in np.flatnonzero(bad):
        R[e] = _axis_kick(rng, 20.0, 170.0) @ R[e]
    R[0] = _axis_kick(rng, 60.0, 60.0) @ R[0]; bad[0] = True
    return n, np.ascontiguousarray(i0), np.ascontiguousarray(i1), R, R_gt, bad


@functools.lru_cache(maxsize=None)
def chain_only(seed=3, n=40):
    """n - 1 edges (k, k + 1), some stored the other way round, shuffled, noisy: the graph is its own spanning tree -> n, i0, i1, R"""
    rng = np.random.default_rng(seed)
    R_gt = synth.so3exp(rng.normal(size=(n, 3)) * 0.8)
    pairs = [(k + 1, k) if rng.random() < 0.3 else (k, k + 1) for k in range(n - 1)]
    pairs = [pairs[k] for k in rng.permutation(n - 1)]
    i0, i1 = np.array(pairs, np.int32).T
    R = np.stack([synth.so3exp(rng.normal(0.0, np.deg2rad(0.5), (1, 3)))[0] @ R_gt[q] @ R_gt[p].T for p, q in pairs])
    return n, np.ascontiguousarray(i0), np.ascontiguousarray(i1), R


@functools.lru_cache(maxsize=None)
def two_components(seed=1):
    """A ring on cameras 0-29 (offsets 1, 2, 3) and a second ring on cameras 30-49 (offsets 1, 2), their edges interleaved in one shuffled list with 12 gross
    outliers; camera 50 has no edge -> n, i0, i1, R, second (E,) bool: the edges of the second component"""
    rng = np.random.default_rng(seed); n = 51
    R_gt = synth.so3exp(rng.normal(size=(n, 3)) * 0.8)
    pairs = [(i, (i + d) % 30) for d in (1, 2, 3) for i in range(30)] + [(30 + i, 30 + (i + d) % 20) for d in (1, 2) for i in range(20)]
    pairs = [pairs[k] for k in rng.permutation(len(pairs))]
    i0, i1 = np.array(pairs, np.int32).T
    R = np.stack([synth.so3exp(rng.normal(0.0, np.deg2rad(0.2), (1, 3)))[0] @ R_gt[q] @ R_gt[p].T for p, q in pairs])
    for e in rng.choice(len(pairs), 12, replace=False):
        R[e] = _axis_kick(rng, 20.0, 170.0) @ R[e]
    return n, np.ascontiguousarray(i0), np.ascontiguousarray(i1), R, i0 >= 30


# the ring60 seeds of the GPU tests (tests/test_rot_l1_cpu.py guards them and lists their figures); WRONG_SUBTREE_SEED's tree start has a median error > 20 degrees
RING60_SEEDS = (0, 4)
WRONG_SUBTREE_SEED = 4


@functools.lru_cache(maxsize=None)
def dense_result(name, seed, root, K):
    """l1_irls(dense) on a named fixture, computed once per session.  K = 0: defaults; K > 0: exactly K iterations (step_tolerance = 0)."""
    fx = fixture(name, seed)
    opt = dict(max_iterations=K, step_tolerance=0.0) if K else {}
    return l1_irls(fx[0], fx[1], fx[2], fx[3], root, "dense", **opt)


def fixture(name, seed=None):
    if name == "ring60":
        return ring60(seed)
    if name == "ring350":
        return ring350(seed or 0)
    return {"complete24": complete24, "chain_only": chain_only, "two_components": two_components, "edge_cases": VR.edge_cases}[name]()
