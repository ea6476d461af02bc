"""A Gram task shared by the waves of a workgroup (ba_kernels.h: schur_gram_task<..., SPLIT = true>; gram_path.h: the waves per task of a launch, SSFM_GRAM_SPLIT): wave w walks
its share of the task's sub-chunks (csrc/gram_path.h: gram_share) through the point pass and the loop, the blocks and the cameras' vectors leave once per task as the sum of the
waves' LDS slices.  Same LM run as one wave per task (SSFM_GRAM_SPLIT=1, the kernel as it was) and as the oracle, on the problems of tests/test_gram_fused_gpu.py --
every instantiation a problem can reach, the unfused three-tile class with k_point_lin in front included -- and on every shape of a share:

  101 points (13 sub-chunks, the last partial): 7 + 6 on two waves, 5 + 4 + 4 on three, 4 + 3 + 3 + 3 on four;
  25 points on four waves: one sub-chunk each, the last with a single point;
  8 points (one sub-chunk) on two and three waves: every wave but the first has an EMPTY share, writes zeros and still takes part in the emission.

No `rejected_steps` case at 1e-5: two identical solves of that start scatter by more than that without any split (profiles/r10_notes.md)."""
import dataclasses
import re

import numpy as np
import pytest

from spherical_sfm_amd import synth

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def point_rel_err(a, b):
    used = np.linalg.norm(b, axis=1) > 0
    return (np.linalg.norm(a[used] - b[used], axis=1) / np.linalg.norm(b[used], axis=1)).max()


def _fixed_points(p, frac=0.02, seed=3):
    rng = np.random.default_rng(seed)
    pt_fixed = p.pt_fixed.copy(); pt_fixed[rng.choice(len(pt_fixed), size=max(1, int(frac * len(pt_fixed))), replace=False)] = 1
    return dataclasses.replace(p, pt_fixed=pt_fixed)


def _circle40(Np, K):
    return synth.make_circle(40, Np, K, spherical=False, check_in_frame=False, xy_range=0.25)


# name -> (problem, planner knobs, waves per task to force besides 1, fused point pass?)
CASES = {
    "6dof_K6": (lambda: _circle40(4040, 6), {"SSFM_GRAM_PTS": "192"}, (2, 3, 4), True),
    "6dof_K6_short": (lambda: _circle40(4000, 6), {}, (2, 4), True),
    "6dof_K3": (lambda: _circle40(4000, 3), {"SSFM_GRAM_PTS": "192"}, (2, 3), True),
    "6dof_K5": (lambda: _circle40(6000, 5), {"SSFM_GRAM_PTS": "192"}, (2, 4), True),
    "6dof_K8": (lambda: _circle40(4000, 8), {"SSFM_GRAM_PTS": "192"}, (2, 4), False),
    "spherical": (lambda: synth.make_circle(48, 7200, 6, spherical=True), {"SSFM_GRAM_PTS": "192"}, (2, 3), True),
    "spherical_K4": (lambda: synth.make_circle(48, 4800, 4, spherical=True), {}, (2, 4), True),
    "spherical_K8": (lambda: synth.make_circle(48, 4848, 8, spherical=True, check_in_frame=False, xy_range=0.25), {"SSFM_GRAM_PTS": "192"}, (2, 3), True),
    "6dof_free_focal": (lambda: synth.make_circle(48, 1200, 6, focal_fixed=False, spherical=False), {"SSFM_GRAM_MIN_RUN": "8"}, (2, 4), True),
    "hard_start": (lambda: synth.make_circle(60, 480, 6, spherical=True, rot_noise_deg=12.0, point_noise=0.3), {"SSFM_GRAM_MIN_RUN": "8"}, (2, 3), True),
    "fixed_points": (lambda: _fixed_points(_circle40(6000, 6)), {"SSFM_GRAM_PTS": "192"}, (2, 4), True),
}


def _plan_knobs(monkeypatch, knobs):
    monkeypatch.setenv("SSFM_NO_PLAN_CACHE", "1")
    monkeypatch.setenv("SSFM_GRAM_MODEL", "0")                            # keep every group that qualifies, however small the problem
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    for k in ("SSFM_GRAM_FUSE", "SSFM_LM_SPECULATE", "SSFM_DETERMINISTIC", "SSFM_GRAM_SPLIT", "SSFM_PLAN_TIMING"):
        monkeypatch.delenv(k, raising=False)


def _same_run(s, s0):
    return (s["termination"] == s0["termination"] and s["iterations"] == s0["iterations"]
            and s["num_successful_steps"] == s0["num_successful_steps"] and s["num_unsuccessful_steps"] == s0["num_unsuccessful_steps"])


def _kernels(ba, ctx, p):
    adj = ba.BundleAdjuster(ctx, p); adj.set_profiling(True); st = adj.run(); kt = adj.kernel_times(); adj.close()
    return st, kt


@pytest.mark.parametrize("name", sorted(CASES))
def test_split_task_changes_nothing_but_the_shape_of_the_launch(gpu_ctx, oracle, monkeypatch, name):
    from spherical_sfm_amd import ba
    make, knobs, splits, fused = CASES[name]
    _plan_knobs(monkeypatch, knobs)
    p = make()
    info = ba.plan(p)[0]
    assert info["num_observations_grouped"] == info["num_observations_used"] == len(p.obs_cam), info
    bar = 1e-5 if name == "hard_start" else 1e-8

    monkeypatch.setenv("SSFM_GRAM_SPLIT", "1")
    c0, p0, f0, s0 = ba.optimize(gpu_ctx, p)
    ocams, opts, of, os_ = oracle.ba_solve(p)
    for W in splits:
        monkeypatch.setenv("SSFM_GRAM_SPLIT", str(W))
        cams, pts, f, s = ba.optimize(gpu_ctx, p)
        print(f"{name}: {W} waves per task: iterations {s['iterations']} accepted {s['num_successful_steps']} rejected {s['num_unsuccessful_steps']}; "
              f"against one wave: cameras {rel_err(cams, c0):.2e} points {point_rel_err(pts, p0):.2e} focal {abs(f - f0) / f0:.2e}; "
              f"against the oracle: cost {abs(s['final_cost'] - os_['final_cost']) / os_['final_cost']:.2e} cameras {rel_err(cams, ocams):.2e} "
              f"points {point_rel_err(pts, opts):.2e}")
        assert _same_run(s, s0), (W, s, s0)
        assert rel_err(cams, c0) <= bar and point_rel_err(pts, p0) <= bar and abs(f - f0) <= bar * f0
        # the oracle, at the tolerances of tests/test_gram_fused_gpu.py
        assert s["termination"] == os_["termination"] and abs(s["iterations"] - os_["iterations"]) <= 1 and s["pcg_iterations_total"] == 0
        assert abs(s["final_cost"] - os_["final_cost"]) <= 1e-7 * os_["final_cost"]
        assert rel_err(cams, ocams) <= 1e-5 and abs(f - of) <= 1e-5 * of
        assert point_rel_err(pts, opts) <= 1e-4

    # launch accounting with the split forced: one Gram launch per linearisation, k_point_lin only in front of the unfused kernel
    st, kt = _kernels(ba, gpu_ctx, p)
    assert kt["k_schur_gram"]["launches"] == st["num_linearizations"]
    assert ("k_point_lin" not in kt) == fused, sorted(kt)


def test_split_of_the_unfused_kernel(gpu_ctx, monkeypatch):
    """SSFM_GRAM_FUSE=0: k_point_lin, then the unfused kernel of the two-tile class with its task split"""
    from spherical_sfm_amd import ba
    make, knobs, splits, _ = CASES["6dof_K6"]
    _plan_knobs(monkeypatch, knobs)
    p = make()
    monkeypatch.setenv("SSFM_GRAM_FUSE", "0")
    monkeypatch.setenv("SSFM_GRAM_SPLIT", "1")
    c0, p0, f0, s0 = ba.optimize(gpu_ctx, p)
    for W in splits:
        monkeypatch.setenv("SSFM_GRAM_SPLIT", str(W))
        cams, pts, f, s = ba.optimize(gpu_ctx, p)
        print(f"unfused, {W} waves per task: cameras {rel_err(cams, c0):.2e} points {point_rel_err(pts, p0):.2e}")
        assert _same_run(s, s0), (W, s, s0)
        assert rel_err(cams, c0) <= 1e-8 and point_rel_err(pts, p0) <= 1e-8 and abs(f - f0) <= 1e-8 * f0
    st, kt = _kernels(ba, gpu_ctx, p)
    assert kt["k_point_lin"]["launches"] == st["num_linearizations"] == kt["k_schur_gram"]["launches"], sorted(kt)


def test_deterministic_mode_stays_bit_identical_with_the_knob_set(gpu_ctx, monkeypatch):
    """SSFM_DETERMINISTIC=1 keeps one wave per task whatever SSFM_GRAM_SPLIT says: two solves agree bit for bit, and with the solve without the knob"""
    from spherical_sfm_amd import ba
    make, knobs, _, _ = CASES["6dof_K6_short"]
    _plan_knobs(monkeypatch, knobs)
    p = make()
    monkeypatch.setenv("SSFM_DETERMINISTIC", "1")
    ref = ba.optimize(gpu_ctx, p)
    monkeypatch.setenv("SSFM_GRAM_SPLIT", "2")
    a = ba.optimize(gpu_ctx, p)
    b = ba.optimize(gpu_ctx, p)
    for x, y in ((a, b), (a, ref)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] and x[3]["final_cost"] == y[3]["final_cost"] and x[3]["iterations"] == y[3]["iterations"]


def test_the_rule_splits_a_small_problem(gpu_ctx, monkeypatch, capfd):
    """Knob unset: 80 tasks of 7 and 6 sub-chunks on a chip that holds 8 waves of this kernel per CU -> the rule gives every task 4 waves (it says so under
    SSFM_PLAN_TIMING), and the run is the run of one wave per task"""
    from spherical_sfm_amd import ba
    make, knobs, _, _ = CASES["6dof_K6_short"]
    _plan_knobs(monkeypatch, knobs)
    p = make()
    monkeypatch.setenv("SSFM_GRAM_SPLIT", "1")
    c0, p0, f0, s0 = ba.optimize(gpu_ctx, p)
    monkeypatch.delenv("SSFM_GRAM_SPLIT")
    monkeypatch.setenv("SSFM_PLAN_TIMING", "1")
    capfd.readouterr()
    cams, pts, f, s = ba.optimize(gpu_ctx, p)
    err = capfd.readouterr().err
    chosen = [int(w) for w in re.findall(r"gram split: class \d+, \d+ tasks, longest \d+ sub-chunks: (\d+) waves per task", err)]
    print("waves per task chosen by the rule:", chosen)
    assert chosen and all(1 < w <= 4 for w in chosen), err[-2000:]
    assert _same_run(s, s0)
    assert rel_err(cams, c0) <= 1e-8 and point_rel_err(pts, p0) <= 1e-8 and abs(f - f0) <= 1e-8 * f0
