"""CPU side of the pairwise front end (ssfm_pairwise_from_features): exported symbols, the argument checks that refuse before anything touches a device (they
come before the context is looked at, so they can be made without one), the resources of the hand-over kernels read from the built code object, and the host-only
functions of the C++ mirror in a stand-alone program under ASan + UBSan.  No kernel is launched here.  (The refusal of a context that carries a communicator
needs a context, hence a device: tests/test_pairwise_front_gpu.py.)"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from spherical_sfm_amd import _lib, match, ransac
from spherical_sfm_amd._lib import c_double_p, c_float_p, c_i32_p, c_i64_p, c_u32_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIB = os.path.join(ROOT, "spherical_sfm_amd", "libssfm_hip.so")


def test_new_symbols_are_exported():
    L = _lib.lib()
    for s in ("ssfm_pairwise_from_features", "ssfm_pairwise_front_last_kernel_ms"):
        assert hasattr(L, s) and s in _lib.DECLARED_SYMBOLS
    from spherical_sfm_amd import pairwise
    assert callable(pairwise.pairwise_from_features)
    assert L.ssfm_pairwise_front_last_kernel_ms(None, None) == -1


def _call(fp, descs, rays, f0, f1, mo, outputs=True, skip=None):
    """the C call without a context: every argument check precedes the look at the context -> (rc, message)"""
    P = len(f0)
    need = np.zeros(2, np.int64); acc = np.zeros(4, np.int32); R = np.zeros(36); nin = np.zeros(4, np.int32); ptr = np.zeros(5, np.int32)
    i0 = np.zeros(8, np.int32); i1 = np.zeros(8, np.int32)
    outs = dict(need=need.ctypes.data_as(c_i64_p), acc=acc.ctypes.data_as(c_i32_p), R=R.ctypes.data_as(c_double_p), nin=nin.ctypes.data_as(c_i32_p),
                ptr=ptr.ctypes.data_as(c_i32_p), i0=i0.ctypes.data_as(c_i32_p), i1=i1.ctypes.data_as(c_i32_p))
    if skip:
        outs[skip] = None
    ro = ransac.default_options(min_num_inliers=10)
    rc = _lib.lib().ssfm_pairwise_from_features(
        None, len(fp) - 1, fp.ctypes.data_as(c_i32_p), descs.ctypes.data_as(c_float_p), rays.ctypes.data_as(c_double_p), P, f0.ctypes.data_as(c_i32_p),
        f1.ctypes.data_as(c_i32_p), C.byref(mo), C.byref(ro), C.c_double(1e-5), C.c_int64(4), C.c_int64(8), outs["need"], outs["acc"], outs["R"], outs["nin"],
        outs["ptr"], outs["i0"], outs["i1"], None, None, None)
    return rc, (_lib.lib().ssfm_last_error(None) or b"").decode()


def test_argument_checks_refuse_before_any_launch():
    fp = np.array([0, 3, 5], np.int32); descs = np.zeros((5, 8), np.float32); rays = np.ones((5, 3)); f0 = np.array([0], np.int32); f1 = np.array([1], np.int32)
    ok = match.default_options(dim=8)
    for bad0, bad1 in ((np.array([2], np.int32), f1), (f0, np.array([-1], np.int32))):
        rc, msg = _call(fp, descs, rays, bad0, bad1, ok)
        assert rc == -1 and "frame index out of range" in msg
    rc, msg = _call(np.array([0, 3, 2], np.int32), descs, rays, f0, f1, ok)
    assert rc == -1 and "feat_ptr must ascend" in msg
    rc, msg = _call(np.array([1, 3, 5], np.int32), descs, rays, f0, f1, ok)
    assert rc == -1 and "feat_ptr[0]" in msg
    rc, msg = _call(fp, descs, rays, f0, f1, match.default_options(dim=6))
    assert rc == -1 and "multiple of 4" in msg
    for ratio in (0.0, -0.5, float("nan"), float("inf")):
        rc, msg = _call(fp, descs, rays, f0, f1, match.default_options(dim=8, ratio=ratio))
        assert rc == -1 and "ratio" in msg
    for skip in ("need", "acc", "R", "nin", "ptr", "i0", "i1"):
        rc, msg = _call(fp, descs, rays, f0, f1, ok, skip=skip)
        assert rc == -1 and "are required" in msg
    rc, msg = _call(fp, descs, rays, f0, f1, ok)                            # everything in order: only now the missing context is noticed
    assert rc == -1 and "ctx is null" in msg
    assert all(m.startswith("ssfm_pairwise_from_features") for m in (msg,))


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(KR.READELF)), reason="needs the built library and llvm-readelf")
def test_hand_over_kernels_have_no_scratch():
    ks = {k["short"]: k for k in KR.kernels(LIB).values()}
    for want in ("k_front_gather", "k_front_count", "k_front_scan", "k_front_compact"):
        names = [n for n in ks if n.startswith(want) or ("::" + want) in n]
        assert names, (want, [n for n in ks if "front" in n])
        for n in names:
            k = ks[n]
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k


def test_mirror_host_functions_under_sanitizers(tmp_path):
    """find_largest_connected_component and read_features (csrc/shim/tools_host.cpp) on hand-made cases (tests/native/front_tools_check.cpp): two components of
    equal size (the first wins), an isolated trailing keyframe, an empty match list, renumbering; features.dat read back without a matches.dat.  ASan + UBSan."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "front_tools_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "front_tools_check.cpp"),
                         os.path.join(ROOT, "spherical_sfm_amd", "csrc", "shim", "tools_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    work = tmp_path / "tracks"; work.mkdir()
    run = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FRONT_TOOLS_CHECK ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr
