"""CPU side of the five-point front end (ssfm_pairwise5_from_features): the exported symbol, its Python wrapper, and the argument checks that refuse before
anything touches a device (they come before the context is looked at, so they can be made without one).  No kernel is launched here.  (The hand-over kernels'
resources are held by tests/test_pairwise_front_cpu.py, which matches every k_front_ instantiation; the refusal of a context that carries a communicator needs
a context, hence a device: tests/test_pairwise5_front_gpu.py.)"""
import ctypes as C

import numpy as np

from spherical_sfm_amd import _lib, match, ransac
from spherical_sfm_amd._lib import c_double_p, c_float_p, c_i32_p, c_i64_p

WHO = "ssfm_pairwise5_from_features"


def test_the_symbol_is_exported_and_declared():
    L = _lib.lib()
    assert hasattr(L, WHO) and WHO in _lib.DECLARED_SYMBOLS
    from spherical_sfm_amd import pairwise
    assert callable(pairwise.pairwise5_from_features) and callable(pairwise.pairwise5_from_features_raw)


def _call(fp, descs, rays, f0, f1, mo, skip=None):
    """the C call without a context: every argument check precedes the look at the context -> (rc, message)"""
    P = len(f0)
    need = np.zeros(2, np.int64); acc = np.zeros(4, np.int32); R = np.zeros(36); t = np.zeros(12); E = np.zeros(36); nin = np.zeros(4, np.int32)
    ptr = np.zeros(5, np.int32); i0 = np.zeros(8, np.int32); i1 = np.zeros(8, np.int32)
    outs = dict(need=need.ctypes.data_as(c_i64_p), acc=acc.ctypes.data_as(c_i32_p), R=R.ctypes.data_as(c_double_p), t=t.ctypes.data_as(c_double_p),
                E=E.ctypes.data_as(c_double_p), nin=nin.ctypes.data_as(c_i32_p), ptr=ptr.ctypes.data_as(c_i32_p), i0=i0.ctypes.data_as(c_i32_p),
                i1=i1.ctypes.data_as(c_i32_p))
    if skip:
        outs[skip] = None
    ro = ransac.default_options(min_num_inliers=10)
    rc = _lib.lib().ssfm_pairwise5_from_features(
        None, len(fp) - 1, fp.ctypes.data_as(c_i32_p), descs.ctypes.data_as(c_float_p), rays.ctypes.data_as(c_double_p), P, f0.ctypes.data_as(c_i32_p),
        f1.ctypes.data_as(c_i32_p), C.byref(mo), C.byref(ro), C.c_double(1e-5), C.c_int64(4), C.c_int64(8), outs["need"], outs["acc"], outs["R"], outs["t"], outs["E"],
        outs["nin"], outs["ptr"], outs["i0"], outs["i1"], None, None, None)
    return rc, (_lib.lib().ssfm_last_error(None) or b"").decode()


def test_argument_checks_refuse_before_any_launch():
    fp = np.array([0, 3, 5], np.int32); descs = np.zeros((5, 8), np.float32); rays = np.ones((5, 3)); f0 = np.array([0], np.int32); f1 = np.array([1], np.int32)
    ok = match.default_options(dim=8)
    msgs = []
    for bad0, bad1 in ((np.array([2], np.int32), f1), (f0, np.array([-1], np.int32))):
        rc, msg = _call(fp, descs, rays, bad0, bad1, ok); msgs.append(msg)
        assert rc == -1 and "frame index out of range" in msg
    rc, msg = _call(np.array([0, 3, 2], np.int32), descs, rays, f0, f1, ok); msgs.append(msg)
    assert rc == -1 and "feat_ptr must ascend" in msg
    rc, msg = _call(fp, descs, rays, f0, f1, match.default_options(dim=6)); msgs.append(msg)
    assert rc == -1 and "multiple of 4" in msg
    for ratio in (0.0, -0.5, float("nan"), float("inf")):
        rc, msg = _call(fp, descs, rays, f0, f1, match.default_options(dim=8, ratio=ratio)); msgs.append(msg)
        assert rc == -1 and "ratio" in msg
    for skip in ("need", "acc", "R", "t", "nin", "ptr", "i0", "i1"):                 # t is required like the others
        rc, msg = _call(fp, descs, rays, f0, f1, ok, skip=skip); msgs.append(msg)
        assert rc == -1 and "are required" in msg and " t," in msg
    for skip in (None, "E"):                                                       # everything in order (E = NULL is): only now the missing context is noticed
        rc, msg = _call(fp, descs, rays, f0, f1, ok, skip=skip); msgs.append(msg)
        assert rc == -1 and "ctx is null" in msg
    assert all(m.startswith(WHO + ":") for m in msgs), msgs
