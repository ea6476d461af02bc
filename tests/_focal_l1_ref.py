"""Test-only restatement of ssfm_focal_search_l1 (include/ssfm.h) in numpy over the oracle's pieces, and the fixtures tests/test_focal_l1_cpu.py and
tests/test_focal_l1_gpu.py share.

* transform: the transform_image_matches step as _view_graph_ref.oracle_cost_tree takes it.
* trial: one trial focal -- transform, then _rot_l1_ref.l1_irls (dense) with the search's defaults, then both costs; the tree cost of
  ssfm_focal_search_graph beside them.
* F60(s) / F24: make_uncalibrated_loop rings (true focal 1000, guessed 1300) with 15 % of the edges rotated by a further 20-170 degrees, cameras renumbered and
  the list shuffled; trial focals linspace(600, 1800, 25), which holds 1000."""
import functools

import numpy as np

from spherical_sfm_amd import synth

import _rot_l1_ref as RR
import _view_graph_ref as VR
from _uncalib_graph import make_uncalibrated_loop

FOCAL_TRUE, FOCAL_GUESS = 1000.0, 1300.0
FOCALS = np.linspace(600.0, 1800.0, 25)
DEFAULTS = dict(RR.DEFAULTS, max_iterations=10)
CUT = RR.CUT


def transform(O, R_rel, focal, focal_guess, inward=False):
    T = np.diag([focal / focal_guess, focal / focal_guess, 1.0])
    Rn = np.zeros_like(R_rel)
    for k in range(len(R_rel)):
        E = O.make_spherical_essential_matrix(R_rel[k], inward)
        r, _ = O.decompose_spherical_essential_matrix(T @ E @ T, inward)
        Rn[k] = synth.so3exp(np.asarray(r)[None])[0]
    return Rn


def trial(O, n, i0, i1, R_rel, focal, focal_guess=FOCAL_GUESS, root=0, **options):
    """-> dict: matches (E,3,3), rotations, residual, iterations, cost (sum |v_e|), get_cost (at the L1 rotations), tree_cost (at the tree chain)"""
    o = dict(DEFAULTS); o.update(options)
    Rn = transform(O, R_rel, focal, focal_guess)
    R, res, s = RR.l1_irls(n, i0, i1, Rn, root, "dense", **o)
    tree = VR.chain_tree(n, VR.bfs_tree(n, i0, i1, root), Rn)
    return dict(matches=Rn, rotations=R, residual=res, iterations=s["iterations"], cost=s["final_cost"], get_cost=O.get_cost(R, i0, i1, Rn),
                tree_cost=O.get_cost(tree, i0, i1, Rn))


def _corrupted_ring(O, n, max_offset, s):
    i0, i1, R, _ = make_uncalibrated_loop(O, n, max_offset, focal_true=FOCAL_TRUE, focal_guess=FOCAL_GUESS, noise_deg=0.05, seed=s)
    E = len(i0)
    rng = np.random.default_rng(s + 100)
    bad = rng.choice(E, int(round(0.15 * E)), replace=False)
    R = R.copy()
    for e in bad:
        R[e] = RR._axis_kick(rng, 20.0, 170.0) @ R[e]
    perm = rng.permutation(n); order = rng.permutation(E)
    mask = np.zeros(E, bool); mask[bad] = True
    return (n, np.ascontiguousarray(perm[i0][order].astype(np.int32)), np.ascontiguousarray(perm[i1][order].astype(np.int32)), np.ascontiguousarray(R[order]),
            mask[order])


@functools.lru_cache(maxsize=None)
def f60(O, s):
    """60 cameras, offsets 1-5: 300 edges, 45 corrupted -> n, i0, i1, R, corrupted (E,) bool"""
    return _corrupted_ring(O, 60, 5, s)


@functools.lru_cache(maxsize=None)
def f24(O):
    """24 cameras, offsets 1-4, seed 0: 96 edges, 14 corrupted"""
    return _corrupted_ring(O, 24, 4, 0)


@functools.lru_cache(maxsize=None)
def curves(O, s):
    """F60(s) over FOCALS, computed once per session -> tree costs (25,), L1 costs (25,), get_costs (25,)"""
    n, i0, i1, R, _ = f60(O, s)
    out = [trial(O, n, i0, i1, R, f) for f in FOCALS]
    return np.array([t["tree_cost"] for t in out]), np.array([t["cost"] for t in out]), np.array([t["get_cost"] for t in out])


@functools.lru_cache(maxsize=None)
def cut_at_best(O, s):
    """F60(s) at the true focal (the L1 argmin, which test_focal_l1_cpu.py guards), the full 30 iterations of ssfm_rot_l1_init -> matches, residuals"""
    n, i0, i1, R, _ = f60(O, s)
    Rn = transform(O, R, FOCAL_TRUE, FOCAL_GUESS)
    _, res, st = RR.l1_irls(n, i0, i1, Rn, 0, "dense")
    return Rn, res, st
