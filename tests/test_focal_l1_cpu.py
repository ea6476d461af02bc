"""CPU side of ssfm_focal_search_l1: the conditions on the fixtures of tests/test_focal_l1_gpu.py (checked with the numpy restatement of tests/_focal_l1_ref.py
alone), the exported symbols and the refusals that come before a context is looked at, and the resources of the kernels of focal_l1.hip read from the built code
object.  No kernel is launched here.

Figures of the F60 fixtures (numpy restatement, 10 iterations, root 0, trial focals linspace(600, 1800, 25), true focal 1000):
  seed   tree argmin   L1 argmin   second-best / best L1 cost   get_cost at the L1 rotations, argmin
   1        600          1000            1.031                        1000
   2        600          1000            1.036                         950
   3        600          1000            1.028                         950
F60(3) at focal 1000 after the 30 iterations of ssfm_rot_l1_init (converged at 15): no corrupted edge below 2 degrees, the largest clean residual 0.21 degrees,
the residual nearest to the cut 0.031 rad away from it."""
import os
import sys

import numpy as np
import pytest

from spherical_sfm_amd import _lib, view_graph

import _focal_l1_ref as FR
import _rot_l1_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIB = os.path.join(ROOT, "spherical_sfm_amd", "libssfm_hip.so")


@pytest.mark.parametrize("seed", [1, 2])
def test_fixture_guard_f60(oracle, seed):
    n, i0, i1, R, bad = FR.f60(oracle, seed)
    assert (n, len(i0), int(bad.sum())) == (60, 300, 45)
    tree, l1, gc = FR.curves(oracle, seed)
    srt = np.sort(l1)
    print(f"F60({seed}): tree argmin {FR.FOCALS[np.argmin(tree)]}, L1 argmin {FR.FOCALS[np.argmin(l1)]}, second / best {srt[1] / srt[0]:.4f}, "
          f"get_cost argmin {FR.FOCALS[np.argmin(gc)]}")
    assert abs(FR.FOCALS[np.argmin(tree)] - FR.FOCAL_TRUE) >= 250.0
    assert FR.FOCALS[np.argmin(l1)] == FR.FOCAL_TRUE
    assert srt[1] > 1.01 * srt[0]


def test_cut_guard_f60(oracle):
    _, l1, _ = FR.curves(oracle, 3)
    assert FR.FOCALS[np.argmin(l1)] == FR.FOCAL_TRUE                                # the best focal of the search is the one cut_at_best solves at
    n, i0, i1, R, bad = FR.f60(oracle, 3)
    _, res, s = FR.cut_at_best(oracle, 3)
    print(f"F60(3) at {FR.FOCAL_TRUE}: {s['iterations']} iterations, nearest residual to the cut {np.abs(res - FR.CUT).min():.3e} rad, "
          f"smallest corrupted {np.rad2deg(res[bad].min()):.2f} deg, largest clean {np.rad2deg(res[~bad].max()):.2f} deg")
    assert s["iterations"] <= 30 and (res >= 0).all()
    assert np.abs(res - FR.CUT).min() > 1e-6
    assert not (res[bad] < FR.CUT).any()


def test_f24_is_what_the_gpu_tests_assume(oracle):
    n, i0, i1, R, bad = FR.f24(oracle)
    assert (n, len(i0), int(bad.sum())) == (24, 96, 14)
    assert 16 * n * 8 + 4 * len(i0) * 8 < 100 * 1024                                # small enough for the LDS placement: FORCE_GLOBAL changes the placement


def test_exports_defaults_and_refusals_before_any_launch():
    L = _lib.lib()
    for sym in ("ssfm_focal_l1_default_options", "ssfm_focal_search_l1"):
        assert hasattr(L, sym) and sym in _lib.DECLARED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "ssfm.h")).read()
    assert "void ssfm_focal_l1_default_options(ssfm_rot_l1_options* o);" in header and "int ssfm_focal_search_l1(ssfm_ctx* ctx," in header
    o = _lib.RotL1OptionsC(); L.ssfm_focal_l1_default_options(o)
    assert {k: getattr(o, k) for k, _ in o._fields_} == FR.DEFAULTS == dict(RR.DEFAULTS, max_iterations=10)
    R = np.tile(np.eye(3), (2, 1, 1)); i0 = np.array([0, 1], np.int32); i1 = np.array([1, 2], np.int32); f = np.array([900.0, 1000.0])
    with pytest.raises(TypeError):
        view_graph.focal_search_l1(None, 3, i0, i1, R, 1000.0, f, no_such_option=1)
    # every refusal is made on the host before the (missing) context is looked at: nothing can have been launched
    for kw, why in ((dict(max_iterations=0), "bad options"), (dict(weight_floor=0.0), "bad options"), (dict(root=3), "root out of range")):
        with pytest.raises(_lib.SsfmError, match="ssfm_focal_search_l1: " + why):
            view_graph.focal_search_l1(None, 3, i0, i1, R, 1000.0, f, **kw)
    with pytest.raises(_lib.SsfmError, match="ssfm_focal_search_l1: camera index out of range"):
        view_graph.focal_search_l1(None, 3, np.array([0, 3], np.int32), i1, R, 1000.0, f)
    with pytest.raises(_lib.SsfmError, match="ssfm_focal_search_l1: bad arguments"):
        view_graph.focal_search_l1(None, 3, i0, i1, R, 1000.0, np.zeros(0))
    with pytest.raises(_lib.SsfmError, match="ssfm_focal_search_l1: ctx is null"):
        view_graph.focal_search_l1(None, 3, i0, i1, R, 1000.0, f)


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(KR.READELF)), reason="needs the built library and llvm-readelf")
def test_focal_l1_kernels_have_no_scratch_and_no_dynamic_stack():
    ks = {k["short"]: k for k in KR.kernels(LIB).values()}
    for want in ("k_focal_l1_start", "k_focal_trials_l1", "k_focal_l1_get_cost"):
        names = [n for n in ks if n == want or n.endswith("::" + want)]
        assert len(names) == 1, (want, [n for n in ks if "focal" in n])
        k = ks[names[0]]
        print(want, {q: k[q] for q in ("vgpr", "sgpr", "scratch", "vgpr_spill", "sgpr_spill", "lds")})
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k
