"""General relative pose (five-point LO-MSAC), the part that needs no GPU: the numpy restatement the GPU tests compare with is itself checked
against ground truth and against the constraints it solves, and the new C entry points exist and check their arguments before they touch a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fivepoint_ref as F
from spherical_sfm_amd import _lib, synth

NEW_SYMBOLS = ["ssfm_ransac5_batch", "ssfm_ransac5_batch_indexed", "ssfm_fivepoint_solver_probe", "ssfm_fivepoint_residual_probe",
               "ssfm_fivepoint_pose_probe", "ssfm_fivepoint_max_lds_rays"]


def _noise_free_samples(count=200):
    rng = np.random.default_rng(11)
    for k in range(count):
        u, v, R, t, E, _ = synth.make_general_pose_problem(12, seed=1000 + k)
        s = rng.choice(12, 5, replace=False)
        yield u[s], v[s], E / np.linalg.norm(E)


def test_restatement_finds_the_true_essential_matrix():
    worst = 0.0
    for u5, v5, E in _noise_free_samples():
        Es = F.solve(u5, v5)
        assert 1 <= len(Es) <= 10
        worst = max(worst, min(F.sign_distance(E, X) for X in Es))
    assert worst <= 1e-8, worst


def test_restatement_solutions_satisfy_the_constraints():
    worst = 0.0
    for u5, v5, _ in _noise_free_samples():
        Es, xyz, w, B = F.solve_full(u5, v5)
        C3 = F.cubics(B)
        for E, s in zip(Es, xyz):
            assert abs(np.linalg.norm(E) - 1.0) <= 1e-12
            epi = np.abs(np.einsum("ni,ij,nj->n", v5, E, u5)).max()                                  # v^T E u = 0 on the five rays
            cub = max(abs(np.linalg.det(E)), np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max())     # the ten cubics on the unit-norm matrix
            worst = max(worst, epi, cub)
            scale = np.linalg.norm(B @ np.append(s, 1.0))
            assert np.abs(F.eval_cubics(C3, *s)).max() <= 1e-9 * max(1.0, scale ** 3)                 # and as polynomials in (x, y, z)
        assert all(a[2] <= b[2] for a, b in zip(xyz, xyz[1:]))                                       # ascending in z
    assert worst <= 1e-9, worst


def test_residual_and_pose_of_the_restatement_on_ground_truth():
    u, v, R, t, E, inl = synth.make_general_pose_problem(50, seed=4)
    assert F.residual(E, u, v).max() <= 1e-20
    Rg, tg, votes = F.pose_from_E(E / np.linalg.norm(E), u, v, np.arange(50))
    assert np.abs(Rg - R).max() <= 1e-12 and np.abs(tg - t).max() <= 1e-12 and votes.max() == 50 and sorted(votes)[-2] == 0


def test_general_motion_generator():
    u, v, R, t, E, inl = synth.make_general_pose_problem(300, noise_px=0.5, outlier_frac=0.3, seed=9)
    assert u.shape == v.shape == (300, 3) and inl.sum() == 210 and abs(np.linalg.norm(t) - 1.0) <= 1e-12
    ang = np.degrees(np.arccos((np.trace(R) - 1) / 2))
    assert 0 <= ang <= 30 + 1e-9
    r = F.residual(E, u, v)
    assert np.sqrt(np.median(r[inl])) * 1000 < 1.5 and np.sqrt(np.median(r[~inl])) * 1000 > 20       # pixels at f = 1000
    # general: t is not the spherical R e_z - e_z
    s = R[:, 2] - np.array([0, 0, 1.0])
    assert np.linalg.norm(np.cross(t, s / np.linalg.norm(s))) > 1e-3


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_harness(outdir, polish_steps=None):
    """tests/native/fivepoint_host.cpp -> a shared library of the device functions, for the CPU"""
    so = os.path.join(str(outdir), "libfp_host%s.so" % ("" if polish_steps is None else "_p%d" % polish_steps))
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "native", "fivepoint_host.cpp")]
    if polish_steps is not None: cmd.append("-DFP_POLISH_STEPS=%d" % polish_steps)
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    L = C.CDLL(so); dp = C.POINTER(C.c_double)
    L.fp_host_solve.argtypes = [dp, dp, dp]; L.fp_host_residual.argtypes = [dp, dp, dp]; L.fp_host_residual.restype = C.c_double
    L.fp_host_decompose.argtypes = [dp, dp, dp, dp]; L.fp_host_cheirality.argtypes = [dp, dp, C.c_double, C.c_double, C.c_double, C.c_double]
    return L


def host_solver_against_restatement(L, count, seed=0):
    """-> (largest distance between a solution of either side and the nearest of the other, samples with different counts, samples left out)"""
    dp = C.POINTER(C.c_double); rng = np.random.default_rng(seed)
    worst, mismatched, left_out = 0.0, 0, 0
    for k in range(count):
        u, v, *_ = synth.make_general_pose_problem(40, noise_px=0.0 if k % 2 == 0 else 0.5, seed=k)
        s = rng.choice(40, 5, replace=False)
        u5 = np.ascontiguousarray(u[s]); v5 = np.ascontiguousarray(v[s]); Es = np.zeros(90)
        c = L.fp_host_solve(u5.ctypes.data_as(dp), v5.ctypes.data_as(dp), Es.ctypes.data_as(dp))
        got = [Es[9 * m:9 * m + 9].reshape(3, 3) for m in range(c)]
        ref, _, w, _ = F.solve_full(u5, v5)
        if F.sample_is_unstable(ref, w): left_out += 1; continue
        if len(got) != len(ref): mismatched += 1; continue
        for E in ref: worst = max(worst, min(F.sign_distance(E, G) for G in got))
        for G in got: worst = max(worst, min(F.sign_distance(E, G) for E in ref))
    return worst, mismatched, left_out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_harness(tmp_path_factory.mktemp("fp_host"))


def test_device_solver_compiled_for_the_cpu_equals_the_restatement(host):
    """the kernels' own solver (csrc/fivepoint_device.h through tests/native/fivepoint_host.cpp) on 300 samples, half noise-free and half with 0.5 px noise: the
    same solution sets as the numpy action-matrix solver.  The bound is the GPU test's (1e-9); 2000 samples of this sequence give 1.7e-11 with the polish and
    1.8e-4 with -DFP_POLISH_STEPS=0 (host_solver_against_restatement(build_host_harness(dir, 0), 2000)), the same counts either way."""
    worst, mismatched, left_out = host_solver_against_restatement(host, 300)
    assert mismatched == 0 and left_out <= 15 and worst <= 1e-9, (worst, mismatched, left_out)
    dp = C.POINTER(C.c_double); Es = np.zeros(90)
    ident = np.ascontiguousarray(np.tile([[0.1, -0.2, 1.0]], (5, 1)))
    assert host.fp_host_solve(ident.ctypes.data_as(dp), ident.ctypes.data_as(dp), Es.ctypes.data_as(dp)) == 0        # rank-deficient: no model


def test_device_pose_pieces_compiled_for_the_cpu_equal_the_restatement(host):
    dp = C.POINTER(C.c_double); p = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(dp)
    for seed in range(20):
        u, v, R, t, E, inl = synth.make_general_pose_problem(30, noise_px=0.5, outlier_frac=0.3, seed=700 + seed)
        E = np.ascontiguousarray(E / np.linalg.norm(E))
        R1 = np.zeros(9); R2 = np.zeros(9); tt = np.zeros(3)
        host.fp_host_decompose(p(E), R1.ctypes.data_as(dp), R2.ctypes.data_as(dp), tt.ctypes.data_as(dp))
        r1, r2, t0 = F.decompose(E)
        assert max(np.abs(R1.reshape(3, 3) - r1).max(), np.abs(R2.reshape(3, 3) - r2).max(), np.abs(tt - t0).max()) <= 1e-12
        # ray 0 may be an inlier: d = v . line is then ~1e-4 of its terms and carries their rounding 1e4 times over, squared: 1e-9 relative, not 1e-12
        assert abs(host.fp_host_residual(p(E), p(u[0]), p(v[0])) - F.residual(E, u[0], v[0])) <= 1e-9 * F.residual(E, u[0], v[0]) + 1e-30
        for Rc, tc in ((r1, t0), (r2, t0), (r1, -t0), (r2, -t0)):
            Rc = np.ascontiguousarray(Rc); tc = np.ascontiguousarray(tc)
            for q in range(30):
                p1, p2 = u[q, :2] / u[q, 2], v[q, :2] / v[q, 2]
                assert bool(host.fp_host_cheirality(p(Rc), p(tc), p1[0], p1[1], p2[0], p2[1])) == F.cheirality(Rc, tc, p1, p2), (seed, q)


def test_new_symbols_exist_and_version():
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.DECLARED_SYMBOLS
    assert L.ssfm_version() == 100                                                                 # unchanged: the ABI only gained entry points
    n = L.ssfm_fivepoint_max_lds_rays()
    assert 1000 < n < 160 * 1024 // 40                                                             # 5 doubles per ray inside one CU's LDS


def test_argument_checks_need_no_device():
    L = _lib.lib()
    dp, ip = _lib.c_double_p, _lib.c_i32_p
    ptr = np.array([0, 5, 10], np.int32); bad = np.array([0, 7, 5], np.int32); U = np.ones((10, 3)); o = _lib.RansacOptionsC()
    L.ssfm_ransac_default_options(C.byref(o))
    E = np.zeros(18); R = np.zeros(18); t = np.zeros(6); mask = np.zeros(10, np.uint8); nin = np.zeros(2, np.int32); sc = np.zeros(2); st = np.zeros(4, np.uint32)
    outs = (E.ctypes.data_as(dp), R.ctypes.data_as(dp), t.ctypes.data_as(dp), mask.ctypes.data_as(_lib.c_u8_p), nin.ctypes.data_as(ip), sc.ctypes.data_as(dp),
            st.ctypes.data_as(_lib.c_u32_p))
    call = lambda ctx, P, p: L.ssfm_ransac5_batch(ctx, P, p.ctypes.data_as(ip), U.ctypes.data_as(dp), U.ctypes.data_as(dp), 1e-6, C.byref(o), *outs)
    err = lambda: L.ssfm_last_error(None)
    assert call(None, 2, ptr) == -1 and b"ctx" in err()                                            # SSFM_ERR_INVALID: NULL ctx
    assert call(None, -1, ptr) == -1 and b"num_pairs" in err()                                     # negative num_pairs
    assert call(None, 2, bad) == -1 and b"ascend" in err()                                         # descending pair_ptr
    fp = np.array([0, 5, 10], np.int32); f0 = np.array([0], np.int32); f1 = np.array([1], np.int32); mp = np.array([0, 5], np.int32); idx = np.arange(5, dtype=np.int32)
    calli = lambda ctx, P: L.ssfm_ransac5_batch_indexed(ctx, 2, fp.ctypes.data_as(ip), U.ctypes.data_as(dp), P, f0.ctypes.data_as(ip), f1.ctypes.data_as(ip),
                                                        mp.ctypes.data_as(ip), idx.ctypes.data_as(ip), idx.ctypes.data_as(ip), C.c_double(1e-6), C.byref(o), *outs)
    assert calli(None, 1) == -1 and b"ctx" in err()
    assert calli(None, -1) == -1 and b"num_pairs" in err()
    assert L.ssfm_fivepoint_solver_probe(None, 10, U.ctypes.data_as(dp), U.ctypes.data_as(dp), 1, idx.ctypes.data_as(ip), E.ctypes.data_as(dp), nin.ctypes.data_as(ip)) == -1
    assert L.ssfm_fivepoint_residual_probe(None, 10, U.ctypes.data_as(dp), U.ctypes.data_as(dp), 1, E.ctypes.data_as(dp), sc.ctypes.data_as(dp)) == -1
    assert L.ssfm_fivepoint_pose_probe(None, 10, U.ctypes.data_as(dp), U.ctypes.data_as(dp), 1, mp.ctypes.data_as(ip), idx.ctypes.data_as(ip), E.ctypes.data_as(dp),
                                       R.ctypes.data_as(dp), t.ctypes.data_as(dp), nin.ctypes.data_as(ip)) == -1
