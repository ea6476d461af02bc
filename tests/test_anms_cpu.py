"""CPU side of ssfm_anms_batch: the properties of the restatement that tests/test_anms_gpu.py compares with (tests/_anms_ref.py: the sort-free set form equals
the literal loop, at least num_to_keep + 1 keypoints survive), the library's host implementation against it, the refusals that come before a context is looked at,
the selection rule of features.select, the resources of the kernels read from the built code object, and the planner + host implementation of anms_host.h in a
stand-alone program under ASan + UBSan.  No kernel is launched here."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from spherical_sfm_amd import _lib, features

import _anms_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIB = os.path.join(ROOT, "spherical_sfm_amd", "libssfm_hip.so")

CASES = [("sift", 1, 0), ("sift", 2, 1), ("sift", 65, 2), ("sift", 300, 3), ("grid", 257, 4), ("signed", 200, 5), ("signed", 33, 6)]


def _keeps(n):
    return sorted({0, 1, n // 4, max(n - 1, 0), n, n + 1})


def test_set_form_equals_the_literal_loop_and_enough_survive():
    for kind, n, seed in CASES:
        for k in _keeps(n):
            xy, r, keep, rad = AR.reference(kind, n, seed, k)
            keep2, rad2 = AR.anms_set_form(xy, r, k)
            assert np.array_equal(keep, keep2) and np.array_equal(rad, rad2), (kind, n, k)
            if n < k:
                assert np.array_equal(keep, np.arange(n)) and (rad == AR.DBL_MAX).all()
            else:
                assert len(keep) >= min(n, k + 1) and len(set(keep.tolist())) == len(keep)
                # sorted order: response descending, equal responses by index
                assert all(r[a] > r[b] or (r[a] == r[b] and a < b) for a, b in zip(keep[:-1], keep[1:]))
            if n == k:
                assert len(keep) == n


def test_inputs_are_strong_enough():
    """What the GPU tests rest on: the tied grid keeps more than num_to_keep + 1, holds duplicated points of radius 0; on the SIFT-like input the subtraction in
    double instead of float changes a radius; the signed input has negative, zero and positive responses."""
    xy, r, keep, rad = AR.reference("grid", 257, 4, 64)
    assert len(keep) > 65 and (rad == 0.0).any() and len(np.unique(r)) < 65
    xy, r, keep, rad = AR.reference("sift", 300, 3, 75)
    assert (AR.anms_literal(xy, r, 75, sub_in_double=True)[1] != rad).sum() >= 1
    xy, r, _, _ = AR.reference("signed", 200, 5, 50)
    assert (r < 0).any() and (r == 0).any() and (r > 0).any() and np.array_equal(r * 8, np.round(r * 8)) and np.abs(r).max() <= 0.75


def test_host_implementation_equals_the_restatement():
    L = _lib.lib()
    for sym in ("ssfm_anms_default_options", "ssfm_anms_batch", "ssfm_anms_batch_host", "ssfm_anms_last_kernel_ms"):
        assert hasattr(L, sym) and sym in _lib.DECLARED_SYMBOLS
    o = _lib.AnmsOptionsC(force_j_chunks=5, reserved=5); L.ssfm_anms_default_options(o)
    assert (o.force_j_chunks, o.reserved) == (0, 0)
    frames = [AR.reference(kind, n, seed, n // 4) for kind, n, seed in CASES] + [AR.reference("sift", 0, 9, 0)]
    keeps = [len(f[1]) // 4 for f in frames]
    for threads in (1, 4):
        got, rad = features.anms_host([f[0] for f in frames], [f[1] for f in frames], keeps, return_radius=True, num_threads=threads)
        for f, g, rr in zip(frames, got, rad):
            assert np.array_equal(g, f[2]) and np.array_equal(rr, f[3])


def test_refusals_before_any_launch():
    xy, r, _, _ = AR.reference("sift", 65, 2, 16)
    # every refusal is made on the host before the (missing) context is looked at: nothing can have been launched
    bad = r.copy(); bad[7] = np.nan
    with pytest.raises(_lib.SsfmError, match="ssfm_anms_batch: NaN response"):
        features.anms(None, [xy], [bad], 16)
    with pytest.raises(_lib.SsfmError, match="ssfm_anms_batch: num_to_keep is negative"):
        features.anms(None, [xy, xy], [r, r], [3, -1])
    with pytest.raises(_lib.SsfmError, match="ssfm_anms_batch: kp_ptr is not ascending"):
        features.anms_flat(None, np.array([0, 65, 40], np.int32), np.concatenate([xy, xy]), np.concatenate([r, r]), [3, 3])
    with pytest.raises(_lib.SsfmError, match="ssfm_anms_batch: bad options"):
        features.anms(None, [xy], [r], 16, force_j_chunks=-1)
    with pytest.raises(_lib.SsfmError, match="ssfm_anms_batch: ctx is null"):
        features.anms(None, [xy], [r], 16)
    with pytest.raises(ValueError):
        features.anms(None, [xy], [r[:-1]], 16)
    with pytest.raises(ValueError):
        features.anms(None, [xy], [r], [1, 2])


def test_select_rule_existing_at_or_above_target_selects_nothing():
    xy, r, _, _ = AR.reference("sift", 65, 2, 16)
    d = np.arange(65 * 4, dtype=np.float32).reshape(65, 4)
    # no frame is live: no call is made at all, so no context is needed
    ptr, descs, pts, keep = features.select(None, [xy, xy], [r, r], [d, d], existing=[4000, 4100], target=4000)
    assert np.array_equal(ptr, [0, 0, 0]) and descs.shape == (0, 4) and pts.shape == (0, 2) and all(len(k) == 0 for k in keep)
    ptr, descs, pts, keep = features.select(None, [xy], [r], None, existing=10, target=10)
    assert np.array_equal(ptr, [0, 0]) and descs is None
    # a live frame goes to the library with ntokeep = target - existing: with no context the call is refused there, after its own checks
    with pytest.raises(_lib.SsfmError, match="ctx is null"):
        features.select(None, [xy, xy], [r, r], None, existing=[4000, 3999], target=4000)
    with pytest.raises(ValueError):
        features.select(None, [xy], [r], None, existing=[1, 2])


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(KR.READELF)), reason="needs the built library and llvm-readelf")
def test_anms_kernels_have_no_scratch_and_no_dynamic_stack():
    ks = {k["short"]: k for k in KR.kernels(LIB).values()}
    for want in ("k_anms_init", "k_anms_radius", "k_anms_select"):
        names = [n for n in ks if n.startswith(want) or ("::" + want) in n]
        assert len(names) == 1, (want, [n for n in ks if "anms" in n])
        k = ks[names[0]]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and not k["dynamic_stack"], k
    # the LDS tile the GPU tests' sizes straddle: 1024 keypoints of 16 bytes
    assert ks["k_anms_radius"]["lds"] == 1024 * 16


def test_planner_and_host_implementation_under_sanitizers(tmp_path):
    """tests/native/anms_host_check.cpp: every (i, j) of every frame covered exactly once by the work list at chunk counts 1 .. 7 and at sizes round the block
    and tile edges; anms_batch_host against a literal loop and the set form written in that file; anms_check's refusals.  ASan + UBSan, host code only."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "anms_host_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tests", "native", "anms_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ANMS_HOST_CHECK ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr
