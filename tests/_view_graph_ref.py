"""Test-only restatement of the view-graph calls (include/ssfm.h: ssfm_triplet_filter, ssfm_view_graph_tree, ssfm_focal_search_graph) in numpy over the oracle's
pieces, and the fixtures the CPU and GPU tests share.

* triplet_filter: the three loops of filter_image_matches (examples/spherical_sfm_tools.cpp:1038-1068) literally, with the oracle's so3ln, for both product orders;
  the records are then put into the order the header defines (i; j by (index1[j], j); k).
* bfs_tree / chain_tree: the spanning tree and the chaining the header defines.
* oracle_cost_tree: loop_constraint_cost_fn (:1142-1159) as tests/test_focal_search_gpu.py::_oracle_cost composes it, with the tree in place of the chain."""
import functools

import numpy as np

from spherical_sfm_amd import synth

ORDER_REFERENCE, ORDER_COMPOSED = 0, 1
THRESH = np.deg2rad(2.0)


def triplet_filter(O, i0, i1, R, thresh, order):
    """-> good (E,) bool, num_triplets, triplets (T,3) in the header's order, errors (T,)"""
    E = len(i0)
    good = np.zeros(E, bool); recs = []
    for i in range(E):
        for j in range(E):
            if i0[j] != i1[i]:
                continue
            for k in range(E):
                if i0[k] != i0[i] or i1[k] != i1[j]:
                    continue
                M = R[i] @ R[j] if order == ORDER_REFERENCE else R[j] @ R[i]
                err = float(np.linalg.norm(O.so3ln(M @ R[k].T)))
                if err < thresh:
                    good[i] = good[j] = good[k] = True
                recs.append((i, int(i1[j]), j, k, err))
    recs.sort(key=lambda r: r[:4])
    tri = np.array([(r[0], r[2], r[3]) for r in recs], np.int32).reshape(-1, 3)
    return good, len(recs), tri, np.array([r[4] for r in recs])


def bfs_tree(n, i0, i1, root):
    """Breadth-first from root; a popped node scans its incident edges in ascending list position and adopts every unseen neighbour.  The arrays of
    spherical_sfm_amd.view_graph.spanning_tree."""
    node = -np.ones(n, np.int32); parent = -np.ones(n, np.int32); edge = -np.ones(n, np.int32); rev = np.zeros(n, np.uint8)
    level = [0]; seen = {root}; node[0] = root; count = 1; head = 0
    while head < count:
        u = int(node[head])
        for e in range(len(i0)):
            if i0[e] == u:
                v, r = int(i1[e]), 0
            elif i1[e] == u:
                v, r = int(i0[e]), 1
            else:
                continue
            if v in seen:
                continue
            seen.add(v)
            node[count] = v; parent[count] = u; edge[count] = e; rev[count] = r; level.append(level[head] + 1); count += 1
        head += 1
    levels = level[-1] + 1
    lp = np.full(n + 1, count, np.int32)
    for k in range(count - 1, -1, -1):
        lp[level[k]] = k
    return dict(num_reached=count, num_levels=levels, node=node, parent=parent, edge=edge, reversed=rev, level_ptr=lp)


def chain_tree(n, tree, rel):
    rot = np.tile(np.eye(3), (n, 1, 1))
    for k in range(1, tree["num_reached"]):
        Re = rel[tree["edge"][k]]
        rot[tree["node"][k]] = (Re.T if tree["reversed"][k] else Re) @ rot[tree["parent"][k]]
    return rot


def oracle_cost_tree(O, n, i0, i1, R_rel, focal, focal_guess, root=0, inward=False):
    T = np.diag([focal / focal_guess, focal / focal_guess, 1.0])
    Rn = np.zeros_like(R_rel)
    for k in range(len(i0)):                                                     # transform_image_matches
        E = O.make_spherical_essential_matrix(R_rel[k], inward)
        r, _ = O.decompose_spherical_essential_matrix(T @ E @ T, inward)
        Rn[k] = synth.so3exp(np.asarray(r)[None])[0]
    rot = chain_tree(n, bfs_tree(n, i0, i1, root), Rn)
    return O.get_cost(rot, i0, i1, Rn), rot


# ---- fixtures shared by tests/test_view_graph_cpu.py (the guard) and tests/test_view_graph_gpu.py ---------------------------------------------------------------

def _noise(rng, deg):
    return synth.so3exp(rng.normal(0.0, np.deg2rad(deg), (1, 3)))[0]


def _kick(rng, deg):
    a = rng.normal(size=3); a *= np.deg2rad(deg) / np.linalg.norm(a)
    return synth.so3exp(a[None])[0]


@functools.lru_cache(maxsize=None)
def complete_graph(seed=4):
    """Complete graph on 12 cameras: 66 edges (a < b), 220 triplets; non-coaxial ground-truth rotations of 10-40 degrees, 0.05 degrees of noise per edge, 6 edges
    rotated by a further 20 degrees -> n, i0, i1, R (E,3,3), corrupted (6,)"""
    rng = np.random.default_rng(seed); n = 12
    ax = rng.normal(size=(n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    R_gt = synth.so3exp(ax * np.deg2rad(rng.uniform(10.0, 40.0, (n, 1))))
    i0, i1 = np.array([(a, b) for a in range(n) for b in range(a + 1, n)], np.int32).T
    R = np.stack([_noise(rng, 0.05) @ R_gt[b] @ R_gt[a].T for a, b in zip(i0, i1)])
    bad = np.sort(rng.choice(len(i0), 6, replace=False))
    for e in bad:
        R[e] = _kick(rng, 20.0) @ R[e]
    return n, np.ascontiguousarray(i0), np.ascontiguousarray(i1), R, bad


@functools.lru_cache(maxsize=None)
def _ring_clean(O):
    from _uncalib_graph import make_uncalibrated_loop
    return make_uncalibrated_loop(O, 40, 3, focal_true=1000.0, focal_guess=1300.0)


def ring(O, seed=2):
    """tests/_uncalib_graph.make_uncalibrated_loop: 40 cameras, offsets 1-3 (rotations as estimated at the guessed focal 1300, true 1000), 4 edges rotated by a
    further 20 degrees -> n, i0, i1, R, corrupted (4,)"""
    i0, i1, R, _ = _ring_clean(O)
    rng = np.random.default_rng(seed)
    bad = np.array([7, 37, 67, 97])                                              # far apart: no clean edge loses all its triplets
    R = R.copy()
    for e in bad:
        R[e] = _kick(rng, 20.0) @ R[e]
    return 40, i0, i1, R, bad


def shuffled_ring(O, seed=5):
    """ring(O) -- its four corrupted edges included -- with the edge list shuffled and the cameras renumbered by a random permutation: no chain (k-1, k) exists
    -> n, i0, i1, R, perm (new number of old camera)"""
    _, i0, i1, R, _ = ring(O)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(40).astype(np.int32); order = rng.permutation(len(i0))
    return 40, np.ascontiguousarray(perm[i0][order]), np.ascontiguousarray(perm[i1][order]), np.ascontiguousarray(R[order]), perm


@functools.lru_cache(maxsize=None)
def edge_cases(seed=9):
    """One unsorted list with everything the join can trip over: camera 0 has 70 out-edges (more than one wave), camera 79 none; edges into camera 0 whose triplets
    reach out-edges beyond lane 63; duplicates, a self loop, two edges stored as (b, a) -> n, i0, i1, R"""
    rng = np.random.default_rng(seed); n = 80
    R_gt = synth.so3exp(rng.normal(size=(n, 3)) * 0.3)
    pairs = [(0, c) for c in range(1, 71)]                                       # out-degree 70
    pairs += [(c, c + 1) for c in range(1, 70, 3)] + [(c, c + 2) for c in range(2, 60, 7)]
    pairs += [(75, 0)] + [(75, c) for c in (3, 40, 66, 70)] + [(75, 79), (76, 0), (76, 69), (76, 70)]
    pairs += [(0, 5), (0, 5), (75, 66), (5, 6)]                                  # duplicates
    pairs += [(7, 7)]                                                            # self loop
    pairs += [(9, 2), (30, 0)]                                                   # stored as (b, a)
    i0, i1 = np.array(pairs, np.int32).T
    R = np.stack([_noise(rng, 0.3) @ R_gt[b] @ R_gt[a].T for a, b in pairs])
    for e in rng.choice(len(pairs), 12, replace=False):
        R[e] = _kick(rng, rng.uniform(1.0, 6.0)) @ R[e]                          # errors on both sides of the threshold
    order = rng.permutation(len(pairs))
    return n, np.ascontiguousarray(i0[order]), np.ascontiguousarray(i1[order]), np.ascontiguousarray(R[order])


@functools.lru_cache(maxsize=None)
def reference_result(O, name, order):
    """the reference loop on a named fixture, computed once per session"""
    fx = {"complete": complete_graph, "edge_cases": edge_cases}[name]() if name != "ring" else ring(O)
    return triplet_filter(O, fx[1], fx[2], fx[3], THRESH, order)
