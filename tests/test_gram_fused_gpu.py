"""The point pass inside the Gram task (ba_kernels.h: schur_gram_task<..., FUSE = true>; ba_solver.hip: LmRun::fuse_lin): when every point of a problem sits in a
signature group, k_schur_gram linearises its own points in a prologue and k_point_lin does not run.  Same LM run as the two-launch path (SSFM_GRAM_FUSE=0), as the
oracle and as the run without speculation, on every tile class and on tasks of one, two and three prologue rounds (a round = 64 points, one lane each).

The three-tile class of 6-dof cameras (K = 7, 8: k_schur_gram<6, 3, 0>) has no fused form -- it would carry more scratch than the unfused kernel -- so a problem with
such tasks keeps k_point_lin: the K = 8 case below checks exactly that.

No 6-dof case with K = 2 (tile class 0, 12 Gram rows): a point enters a problem with >= 3 observations (ba_flatten.h), so no 6-dof task has fewer than 18 rows;
the one-tile class runs on 3-dof cameras (K = 4) instead, and K = 8 there covers the two-tile class: every fused instantiation a problem can reach is run.

The hard start of test_speculative_linearisation_changes_nothing_but_time has runs of 300 / 60 = 5 points with one camera list, below the 8 points of the shortest
possible group (SSFM_GRAM_MIN_RUN >= 8): here it has 480 points (runs of 8), everything else as there.  The CPU oracle rejects no step on it (nor on the 300-point
original), so a second start with 20 degrees of rotation noise -- two rejected steps in the oracle's run -- stands for "the device says no"."""
import dataclasses

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
    """6-dof circle of 40 cameras (9 degrees apart: a narrow anchor window keeps every point in front of its K cameras; the frame check is for 1920 x 1080 rings)"""
    return synth.make_circle(40, Np, K, spherical=False, check_in_frame=False, xy_range=0.25)


# name -> (problem, planner knobs, points per task, fused?).  Points per camera window L = Np / Nc and SSFM_GRAM_PTS decide the task lengths (ba_flatten.h: a run
# is cut into equal parts of whole sub-chunks): L = 100 by default -> 56 + 44; L = 101 / 100 in one task; L = 150 in one task (64 + 64 + 22).
CASES = {
    "6dof_K3": (lambda: _circle40(4000, 3), {"SSFM_GRAM_PTS": "192"}, (100,), True),
    "6dof_K5": (lambda: _circle40(6000, 5), {"SSFM_GRAM_PTS": "192"}, (150,), True),
    "6dof_K6": (lambda: _circle40(4040, 6), {"SSFM_GRAM_PTS": "192"}, (101,), True),
    "6dof_K6_short": (lambda: _circle40(4000, 6), {}, (56, 44), True),
    "6dof_K8": (lambda: _circle40(4000, 8), {"SSFM_GRAM_PTS": "192"}, (100,), False),
    "spherical": (lambda: synth.make_circle(48, 7200, 6, spherical=True), {"SSFM_GRAM_PTS": "192"}, (150,), True),
    "spherical_K4": (lambda: synth.make_circle(48, 4800, 4, spherical=True), {}, (56, 44), True),
    "spherical_K8": (lambda: synth.make_circle(48, 4848, 8, spherical=True, check_in_frame=False, xy_range=0.25), {"SSFM_GRAM_PTS": "192"}, (101,), True),
    "spherical_free_focal": (lambda: synth.make_circle(48, 3360, 6, spherical=True, focal_fixed=False), {}, (40, 30), True),
    "6dof_free_focal": (lambda: synth.make_circle(48, 1200, 6, focal_fixed=False, spherical=False), {"SSFM_GRAM_MIN_RUN": "8"}, (25,), True),
    "fixed_points": (lambda: _fixed_points(_circle40(6000, 6)), {"SSFM_GRAM_PTS": "192"}, (150,), True),
    "hard_start": (lambda: synth.make_circle(60, 480, 6, spherical=True, rot_noise_deg=12.0, point_noise=0.3), {"SSFM_GRAM_MIN_RUN": "8"}, (8,), True),
    "rejected_steps": (lambda: synth.make_circle(60, 480, 6, spherical=True, rot_noise_deg=20.0, point_noise=0.3), {"SSFM_GRAM_MIN_RUN": "8"}, (8,), True),
}


def test_task_lengths_cover_every_prologue_round_count():
    lens = [n for _, _, ns, fused in CASES.values() if fused for n in ns]
    assert any(n < 64 for n in lens) and any(64 < n < 128 and n % 8 for n in lens) and any(n > 128 for n in lens)


def _kernels(ba, ctx, p):
    adj = ba.BundleAdjuster(ctx, p); adj.set_profiling(True); st = adj.run(); kt = adj.kernel_times(); adj.close()
    return st, kt


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_point_pass_changes_nothing_but_the_launches(gpu_ctx, oracle, monkeypatch, name):
    from spherical_sfm_amd import ba
    make, knobs, task_pts, fused = CASES[name]
    monkeypatch.setenv("SSFM_NO_PLAN_CACHE", "1")
    monkeypatch.setenv("SSFM_GRAM_MODEL", "0")                            # keep every group that qualifies, however small the problem
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    for k in ("SSFM_GRAM_FUSE", "SSFM_LM_SPECULATE", "SSFM_DETERMINISTIC"):
        monkeypatch.delenv(k, raising=False)
    p = make()
    info = ba.plan(p)[0]
    assert info["num_observations_grouped"] == info["num_observations_used"] == len(p.obs_cam), info
    hard = name in ("hard_start", "rejected_steps")
    bar = 1e-5 if hard else 1e-8

    cams, pts, f, s = ba.optimize(gpu_ctx, p)
    monkeypatch.setenv("SSFM_GRAM_FUSE", "0")
    c0, p0, f0, s0 = ba.optimize(gpu_ctx, p)
    monkeypatch.delenv("SSFM_GRAM_FUSE")
    print(f"{name}: iterations {s['iterations']} accepted {s['num_successful_steps']} rejected {s['num_unsuccessful_steps']}; against SSFM_GRAM_FUSE=0: "
          f"cameras {rel_err(cams, c0):.2e} points {point_rel_err(pts, p0):.2e}")
    assert s["termination"] == s0["termination"] and s["iterations"] == s0["iterations"]
    assert s["num_successful_steps"] == s0["num_successful_steps"] and s["num_unsuccessful_steps"] == s0["num_unsuccessful_steps"]
    assert rel_err(cams, c0) <= bar and point_rel_err(pts, p0) <= bar and abs(f - f0) <= bar * f0
    if name == "rejected_steps":
        assert s["num_unsuccessful_steps"] > 0                           # what the case is for: the device says no, the speculative launch does not run

    # the oracle, at the tolerances of tests/test_gram_groups_gpu.py
    ocams, opts, of, os_ = oracle.ba_solve(p)
    assert s["termination"] == os_["termination"] and abs(s["iterations"] - os_["iterations"]) <= 1 and s["pcg_iterations_total"] == 0
    assert abs(s["final_cost"] - os_["final_cost"]) <= 1e-7 * os_["final_cost"]
    assert rel_err(cams, ocams) <= 1e-5 and abs(f - of) <= 1e-5 * of
    assert point_rel_err(pts, opts) <= 1e-4

    # every launch waits for the host (the bar of test_speculative_linearisation_changes_nothing_but_time)
    monkeypatch.setenv("SSFM_LM_SPECULATE", "0")
    c1, p1, f1, s1 = ba.optimize(gpu_ctx, p)
    monkeypatch.delenv("SSFM_LM_SPECULATE")
    assert s["termination"] == s1["termination"] and s["iterations"] == s1["iterations"]
    assert s["num_successful_steps"] == s1["num_successful_steps"] and s["num_unsuccessful_steps"] == s1["num_unsuccessful_steps"]
    assert rel_err(cams, c1) <= 1e-5 and point_rel_err(pts, p1) <= 1e-5

    # launch accounting: one Gram launch per linearisation, k_point_lin only where the fused path is not taken
    st, kt = _kernels(ba, gpu_ctx, p)
    assert kt["k_schur_gram"]["launches"] == st["num_linearizations"]
    assert ("k_point_lin" not in kt) == fused, sorted(kt)
    for var in ("SSFM_GRAM_FUSE", "SSFM_DETERMINISTIC"):
        monkeypatch.setenv(var, "0" if var == "SSFM_GRAM_FUSE" else "1")
        st2, kt2 = _kernels(ba, gpu_ctx, p)
        monkeypatch.delenv(var)
        assert kt2["k_point_lin"]["launches"] == st2["num_linearizations"] == kt2["k_schur_gram"]["launches"], (var, sorted(kt2))
