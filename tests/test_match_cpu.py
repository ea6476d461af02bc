"""CPU side of the descriptor matching: the numpy restatement (tests/_match_ref.py) against a plain triple loop, the exported symbols and default
options of the library, and the resources of the distance kernel read from the built code object.  No kernel is launched here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _match_ref as R
from spherical_sfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIB = os.path.join(ROOT, "spherical_sfm_amd", "libssfm_hip.so")


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_overwrite_rule_the_larger_query_index_stays():
    t = np.array([[10.0, 0, 0, 0], [0, 10.0, 0, 0], [0, 0, 10.0, 0]])
    q = np.array([[0, 9.0, 0, 0], [9.5, 0, 0, 0], [0, 9.9, 0, 0], [0, 8.0, 0, 0]])        # queries 0, 2, 3 all go to train 1
    got = R.match_pair(t, q)
    assert got[0].tolist() == [0, 1] and got[1].tolist() == [1, 3]
    assert _same(got, R.match_triple_loop(t, q))


def test_fewer_than_two_train_rows_give_no_matches():
    q = np.ones((3, 4))
    for n0 in (0, 1):
        got = R.match_pair(np.zeros((n0, 4)), q)
        assert len(got[0]) == 0 and len(got[1]) == 0
        assert _same(got, R.match_triple_loop(np.zeros((n0, 4)), q))
    assert len(R.match_pair(np.ones((5, 4)), np.zeros((0, 4)))[0]) == 0


def test_a_tie_never_passes_below_ratio_one():
    t = np.array([[3.0, 0, 0, 0], [0, 3.0, 0, 0], [50.0, 50.0, 0, 0]])
    q = np.zeros((1, 4))
    assert len(R.match_pair(t, q, 0.75)[0]) == 0 and len(R.match_pair(t, q, 1.0)[0]) == 0
    got = R.match_pair(t, q, 1.5)                                                          # ratio >= 1: the lower train index
    assert got[0].tolist() == [0] and got[1].tolist() == [0]
    assert _same(got, R.match_triple_loop(t, q, 1.5))


def test_restatement_equals_the_triple_loop_on_random_small_cases():
    rng = np.random.default_rng(0)
    for s in range(40):
        t = np.rint(rng.uniform(0, 6, (rng.integers(0, 14), 4))); q = np.rint(rng.uniform(0, 6, (rng.integers(0, 9), 4)))     # small integers: many ties
        for ratio in (0.75, 1.0, 1.5):
            assert _same(R.match_pair(t, q, ratio), R.match_triple_loop(t, q, ratio)), (s, ratio)


def test_integer_descriptors_make_the_product_form_exact():
    """the argument of include/ssfm.h: integers 0..255 in 128 bins -> every squared distance is an integer < 2^24, the float32 product form is exact"""
    pool = R.world_pool(600, seed=3)
    a = R.integer_frame(pool, 300, 1)[0]; b = R.integer_frame(pool, 300, 2)[0]
    assert a.max() <= 255 and a.min() >= 0 and np.array_equal(a, np.rint(a))
    g = ((b * b).sum(1)[:, None] + (a * a).sum(1)[None, :] - np.float32(2) * (b @ a.T)).astype(np.float32)               # float32 throughout
    direct = ((b.astype(np.float64)[:, None, :] - a.astype(np.float64)[None, :, :]) ** 2).sum(2)
    assert direct.max() < 2 ** 24 and np.array_equal(g.astype(np.float64), direct)
    nn, _, dist = R.knn2(a, b)
    frac = R.ratio_pass(dist, nn, 0.75).mean()
    assert 0.10 <= frac <= 0.90


def test_new_symbols_are_exported_and_defaults():
    L = _lib.lib()
    for s in ("ssfm_match_default_options", "ssfm_match_pairs", "ssfm_match_knn_probe", "ssfm_match_last_kernel_ms"):
        assert hasattr(L, s) and s in _lib.DECLARED_SYMBOLS
    o = _lib.MatchOptionsC(ratio=-1.0, dim=-1, reserved=7)
    L.ssfm_match_default_options(C.byref(o))
    assert o.ratio == 0.75 and o.dim == 128 and o.reserved == 0                     # spherical_sfm_tools.h:70; SIFT
    assert C.sizeof(_lib.MatchOptionsC) == 16
    from spherical_sfm_amd import match
    assert match.exhaustive_pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] == R.exhaustive_pairs(4)


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(KR.READELF)), reason="needs the built library and llvm-readelf")
def test_distance_kernel_has_no_scratch():
    ks = {k["short"]: k for k in KR.kernels(LIB).values()}
    names = [n for n in ks if n.startswith("k_match_dist") or "::k_match_dist" in n]
    assert names, [n for n in ks if "match" in n]
    for n in names:
        k = ks[n]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k
        assert k["vgpr"] + k["agpr"] <= 512 and k["lds"] <= 160 * 1024, k
