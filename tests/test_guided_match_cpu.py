"""CPU side of guided matching (ssfm_guided_match_pairs): the numpy restatement (tests/_guided_ref.py) against a plain triple loop and against the plain
matcher's restatement, the repeated-structure scene the feature is for, the exported symbols and defaults, spherical_essential against the oracle, and the
resources of k_guided_dist read from the built code object.  No kernel is launched here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _guided_ref as G
import _match_ref as M
from spherical_sfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIB = os.path.join(ROOT, "spherical_sfm_amd", "libssfm_hip.so")


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _small_case(rng):
    """small integer descriptors (many ties) with rays near the optical axis of a 4 degree pair; the band admits roughly half of the entries"""
    n0 = int(rng.integers(0, 14)); n1 = int(rng.integers(0, 9))
    t = np.rint(rng.uniform(0, 6, (n0, 4))); q = np.rint(rng.uniform(0, 6, (n1, 4)))
    u = np.concatenate([rng.uniform(-0.5, 0.5, (n0, 2)), np.ones((n0, 1))], axis=1)
    v = np.concatenate([rng.uniform(-0.5, 0.5, (n1, 2)), np.ones((n1, 1))], axis=1)
    return t, u, q, v


def test_restatement_equals_the_triple_loop_on_random_small_cases():
    rng = np.random.default_rng(0)
    E = G.essential_of_step(4.0)[0]
    admitted = []
    for s in range(40):
        t, u, q, v = _small_case(rng)
        thr2 = float(rng.choice([1e-3, 1e-2, 1e-1]))
        if len(t) and len(q):
            admitted.append(G.cand_mask(u, v, E, thr2).mean())
        for ratio in (0.75, 1.0, 1.5):
            for md in (np.inf, 3.0):
                assert _same(G.guided_pair(t, u, q, v, E, thr2, ratio, md), G.guided_triple_loop(t, u, q, v, E, thr2, ratio, md)), (s, ratio, md)
    assert 0.05 < np.mean(admitted) < 0.95                                            # the mask is neither empty nor full on these cases


def test_ties_lone_candidate_max_distance_zero_E_and_zero_threshold():
    E = G.essential_of_step(4.0)[0]
    u = np.array([[0.0, 0.0, 1.0], [0.01, 0.0, 1.0], [0.0, 0.3, 1.0]])               # rows 0 and 1 lie on the epipolar line y = 0 of the query, row 2 far off it
    v = np.array([[0.05, 0.0, 1.0]])
    thr2 = 1e-4
    assert G.cand_mask(u, v, E, thr2).tolist() == [[True, True, False]]
    t = np.array([[3.0, 0, 0, 0], [0, 3.0, 0, 0], [0.0, 0, 0, 0]]); q = np.zeros((1, 4))    # the nearest row over all (2) is outside the band; 0 and 1 tie
    for ratio in (0.75, 1.0):
        assert len(G.guided_pair(t, u, q, v, E, thr2, ratio)[0]) == 0                # a tie never passes at ratio <= 1
    got = G.guided_pair(t, u, q, v, E, thr2, 1.5)
    assert got[0].tolist() == [0] and got[1].tolist() == [0]                         # ratio > 1: the lower train index
    assert _same(got, G.guided_triple_loop(t, u, q, v, E, thr2, 1.5))
    # a lone candidate is accepted whatever its distance, unless max_distance cuts it
    got = G.guided_pair(t[[0, 2]], u[[0, 2]], q, v, E, thr2)
    assert got[0].tolist() == [0] and got[1].tolist() == [0] and _same(got, G.guided_triple_loop(t[[0, 2]], u[[0, 2]], q, v, E, thr2))
    assert len(G.guided_pair(t[[0, 2]], u[[0, 2]], q, v, E, thr2, max_distance=2.5)[0]) == 0
    assert len(G.guided_triple_loop(t[[0, 2]], u[[0, 2]], q, v, E, thr2, max_distance=2.5)[0]) == 0
    assert G.guided_pair(t[[0, 2]], u[[0, 2]], q, v, E, thr2, max_distance=3.0)[0].tolist() == [0]          # dist1 <= max_distance
    # E = 0: 0 < 0 is "no"; threshold 0: d d < 0 is "no"
    for EE, th in ((np.zeros((3, 3)), thr2), (E, 0.0)):
        assert not G.cand_mask(u, v, EE, th).any()
        assert len(G.guided_pair(t, u, q, v, EE, th, 1.5)[0]) == 0 and len(G.guided_triple_loop(t, u, q, v, EE, th, 1.5)[0]) == 0


def test_a_band_that_admits_everything_is_the_plain_matcher():
    rng = np.random.default_rng(1)
    E = G.essential_of_step(4.0)[0]
    for s in range(40):
        t, u, q, v = _small_case(rng)
        if len(t) < 2:
            continue
        assert G.cand_mask(u, v, E, 1e30).all()
        for ratio in (0.75, 1.0, 1.5):
            assert _same(G.guided_pair(t, u, q, v, E, 1e30, ratio), M.match_pair(t, q, ratio)), (s, ratio)


@pytest.mark.parametrize("seed", range(4))
def test_repeated_structure_is_what_guided_matching_recovers(seed):
    sc = G.repeated_pair(seed)
    S = G.sampson(sc["u"], sc["v"], sc["E"])
    gap = G.band_gap(S, G.THR2)
    assert gap > 1e-9, gap                                                           # observed >= 2e-4: an fp64 predicate cannot disagree with numpy's
    true_S = S[np.arange(len(S)), sc["truth"]]
    assert true_S.max() < G.THR2                                                     # every true pair is inside the band
    pj, pi = M.match_pair(sc["train"], sc["query"], 0.75)
    gj, gi = G.guided_pair(sc["train"], sc["u"], sc["query"], sc["v"], sc["E"], G.THR2, 0.75)
    plain_ok = int((sc["truth"][pi] == pj).sum()); guided_ok = int((sc["truth"][gi] == gj).sum())
    print(f"seed {seed}: band_gap {gap:.3e}, band admits {G.cand_mask(sc['u'], sc['v'], sc['E'], G.THR2).mean():.4f}, plain {len(pj)} ({plain_ok} right), "
          f"guided {len(gj)} ({guided_ok} right), max true Sampson / thr2 {true_S.max() / G.THR2:.3f}")
    assert guided_ok == len(gj)                                                      # no wrong guided match
    assert guided_ok >= 1.5 * len(pj)
    assert not sc["repeated"][pi].any()                                              # Lowe's test over the whole frame keeps the unrepeated half only


def test_new_symbols_are_exported_and_defaults():
    L = _lib.lib()
    for s in ("ssfm_guided_match_default_options", "ssfm_guided_match_pairs", "ssfm_guided_knn_probe", "ssfm_guided_match_last_kernel_ms"):
        assert hasattr(L, s) and s in _lib.DECLARED_SYMBOLS
    o = _lib.GuidedMatchOptionsC(ratio=-1.0, squared_threshold=-1.0, max_distance=-1.0, dim=-1)
    L.ssfm_guided_match_default_options(C.byref(o))
    assert (o.ratio, o.squared_threshold, o.max_distance, o.dim) == (0.75, 0.0, np.inf, 128)
    assert C.sizeof(_lib.GuidedMatchOptionsC) == 24
    assert C.sizeof(_lib.MatchOptionsC) == 16                                        # the plain options are as they were
    from spherical_sfm_amd import match, pairwise
    for name in ("guided_default_options", "guided_match_flat", "guided_match_pairs", "guided_knn_probe", "guided_last_kernel_ms"):
        assert callable(getattr(match, name))
    assert callable(pairwise.guided_rematch)
    d = match.guided_default_options(squared_threshold=G.THR2)
    assert d.squared_threshold == G.THR2 and d.ratio == 0.75


def test_spherical_essential_equals_the_oracle():
    from oracle import oracle as O
    from spherical_sfm_amd import pairwise, synth
    rng = np.random.default_rng(5)
    for k in range(8):
        R = synth.so3exp(rng.normal(0, 0.3, 3))
        for inward in (False, True):
            got = pairwise.spherical_essential(R, inward); want = O.make_spherical_essential_matrix(R, inward)
            assert np.abs(got - want).max() <= 1e-15, (k, inward, np.abs(got - want).max())
    Rs = np.stack([synth.so3exp(rng.normal(0, 0.3, 3)) for _ in range(3)])
    assert np.array_equal(pairwise.spherical_essential(Rs), np.stack([pairwise.spherical_essential(R) for R in Rs]))
    # the scene's own E (built from the camera model) is the outward spherical E of its rotation
    E, R = G.essential_of_step(4.0)
    assert np.abs(E - pairwise.spherical_essential(R)).max() <= 1e-15


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(KR.READELF)), reason="needs the built library and llvm-readelf")
def test_guided_kernel_resources():
    ks = {k["short"]: k for k in KR.kernels(LIB).values()}
    names = [n for n in ks if n.startswith("k_guided_dist") or "::k_guided_dist" in n]
    assert len(names) == 2, [n for n in ks if "guided" in n]                         # the call's form and the probe's
    for n in names:
        k = ks[n]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k
        assert k["vgpr"] + k["agpr"] <= 512 and k["lds"] <= 160 * 1024, k
