"""CPU side of the stereo panorama: ssfm_pano_plan against the float64 restatement of examples/stereo_panorama_tools.cpp:496-616 (tests/_pano_ref.py) -- the
integer columns (pair, theta, phi, col, ok, owner) equal, alpha / tan(phi) / synth_R to 1e-13 absolute (they differ by libm's last bits, the values are O(1)) --
on the three scenes the GPU tests use, the degenerate sizes, the refusals that come before a context is looked at, and the plan, the levelling, the thetas, the
loop trimming and the PPM / .flo readers in a stand-alone program under ASan + UBSan.  No kernel is launched here."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from spherical_sfm_amd import _lib, pano

import _pano_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(s, **opts):
    ref = PR.plan(s["R"], s["t"], s["intr"], s["height"], s["pano_width"], **opts)
    got = pano.plan(s["R"], s["t"], s["intr"], s["width"], s["height"], s["pano_width"], **opts)
    # no decision of the restatement is closer than 1e-9 to its threshold: nothing below hangs on a last bit
    assert ref["margin"] > 1e-9, ref["margin"]
    for k in ("pair", "theta", "phi", "col", "ok", "owner"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    for k in ("alpha", "tan_phi", "synth_R"):
        assert got[k].shape == ref[k].shape and (np.abs(got[k] - ref[k]).max() if got[k].size else 0.0) <= 1e-13, k
    return ref, got


@pytest.mark.parametrize("opts", [dict(num_phi=9, is_loop=1), dict(num_phi=9, is_loop=0), dict(num_phi=1, is_loop=1), dict(num_phi=1, is_loop=0)])
def test_scene1_plan(opts):
    """7 cameras on the unit circle with small noise, 48 x 37 frames, pano_width 193: nine phis and one, loop and open."""
    ref, got = _both(PR.scene1(), **opts)
    assert len(ref["pair"]) >= (1000 if opts["num_phi"] == 9 else 100) and ref["ok"].all()
    owned = (ref["owner"] >= 0).mean()
    assert (owned > 0.8 if opts["is_loop"] else 0.6 < owned < 0.9), owned
    assert ((ref["alpha"] > 0) & (ref["alpha"] < 1)).all()
    if not opts["is_loop"]:
        assert ref["pair"].max() == 5                                       # the last keyframe does not pair with the first


def test_scene2_columns_claimed_twice_go_to_the_highest_pair():
    """12 cameras, tilt sigma 0.6: the projected centres are no longer in angular order, so columns are claimed by more than one pair."""
    ref, got = _both(PR.scene2())
    assert ref["overwrites"] >= 1
    claims = {}
    for j in np.nonzero(got["ok"])[0]:
        claims.setdefault((int(got["phi"][j]), int(got["col"][j])), []).append(int(got["pair"][j]))
    multi = {k: v for k, v in claims.items() if len(v) > 1}
    assert len(multi) >= 1 and all(len(set(v)) == len(v) for v in claims.values())          # a pair claims a column at most once
    for (p, c), v in claims.items():
        assert got["owner"][p, c] == max(v)
    assert (got["owner"] >= 0).sum() == len(claims)


@pytest.mark.parametrize("kind", ["yaw", "pitch"])
def test_scene3_jobs_that_are_not_ok_write_nothing(kind):
    """One camera turned about its own centre (yaw 1.7 rad; pitch 1.1 rad at focal 12): the plane lies behind it on some rows, its jobs are not ok, and the
    column keeps an earlier pair's job or none."""
    ref, got = _both(PR.scene3(kind))
    bad = np.nonzero(got["ok"] == 0)[0]
    assert len(bad) >= 1 and got["ok"].any()
    left = [j for j in bad if got["owner"][got["phi"][j], got["col"][j]] < got["pair"][j]]
    assert len(left) >= 1
    assert all(got["owner"][got["phi"][j], got["col"][j]] != got["pair"][j] for j in bad)       # (a pair has one job per column)


def _raw_plan(s, n, pano_width, capacity, arrays=True, **opts):
    o = pano.options(**opts)
    R = np.ascontiguousarray(s["R"][:n], np.float64); t = np.ascontiguousarray(s["t"][:n], np.float64)
    cap = max(capacity, 1)
    ji = [np.full(cap, -7, np.int32) for _ in range(4)]; ok = np.full(cap, 9, np.uint8); alpha = np.full(cap, -7.0); consts = np.full((cap, 10), -7.0)
    owner = np.full((max(o.num_phi, 1), max(pano_width, 1)), -9, np.int32)
    count = C.c_int32(capacity)
    f, cx, cy = s["intr"]
    ptrs = [a.ctypes.data_as(_lib.c_i32_p) for a in ji] + [ok.ctypes.data_as(_lib.c_u8_p), alpha.ctypes.data_as(_lib.c_double_p), consts.ctypes.data_as(_lib.c_double_p)]
    rc = _lib.lib().ssfm_pano_plan(C.byref(o), n, R.ctypes.data_as(_lib.c_double_p), t.ctypes.data_as(_lib.c_double_p), f, cx, cy, s["width"], s["height"], pano_width,
                                   C.byref(count), *(ptrs if arrays else [None] * 7), owner.ctypes.data_as(_lib.c_i32_p))
    return rc, count.value, ji, owner


def test_degenerate_sizes_and_capacity():
    s = PR.scene1()
    for n in (0, 1):
        for loop in (0, 1):
            rc, count, _, owner = _raw_plan(s, n, 193, 16, is_loop=loop)
            assert (rc, count) == (0, 0) and (owner == -1).all()
            ref = PR.plan(s["R"][:n], s["t"][:n], s["intr"], s["height"], 193, is_loop=loop)
            assert len(ref["pair"]) == 0
    s2 = dict(s, R=s["R"][:2], t=s["t"][:2])
    for loop in (0, 1):
        ref, got = _both(s2, is_loop=loop)
        assert len(ref["pair"]) >= 1 and set(ref["pair"].tolist()) <= ({0, 1} if loop else {0})
    ref, got = _both(dict(s, pano_width=2))                                  # theta_step = 2 pi: two columns
    assert got["owner"].shape == (9, 2)
    # a capacity below the job count: the error code, the needed count, the job arrays untouched, the owner map still written
    full = pano.plan(s["R"], s["t"], s["intr"], s["width"], s["height"], 193)
    need = len(full["pair"])
    rc, count, ji, owner = _raw_plan(s, 7, 193, need - 1)
    assert rc == -1 and count == need and (ji[0] == -7).all() and np.array_equal(owner, full["owner"])
    assert "capacity" in _lib.lib().ssfm_last_error(None).decode()
    rc, count, _, _ = _raw_plan(s, 7, 193, 0, arrays=False)
    assert rc == -1 and count == need
    rc, count, ji, _ = _raw_plan(s, 7, 193, need)
    assert rc == 0 and count == need and np.array_equal(ji[0], full["pair"])


def test_symbols_options_and_refusals_before_any_launch():
    L = _lib.lib()
    for sym in ("ssfm_pano_default_options", "ssfm_pano_plan", "ssfm_pano_synthesize", "ssfm_pano_last_kernel_ms"):
        assert hasattr(L, sym) and sym in _lib.DECLARED_SYMBOLS
    assert C.sizeof(_lib.PanoOptionsC) == 56
    o = pano.options()
    assert (o.num_phi, o.phi_step_deg, o.depth, o.synth_radius, o.synth_focal_factor, o.is_loop, o.subpixel_bits, o.on_device, o.max_slab_bytes) == (9, 1.0, 10.0, 0.5, 1.2, 1, 0, 0, 0)
    with pytest.raises(TypeError):
        pano.options(no_such_option=1)
    s = PR.scene1(); frames = np.zeros((7, 37, 48, 3), np.uint8); flow = np.zeros((7, 37, 48, 2), np.float32)
    # every refusal is made on the host before the (missing) context is looked at: nothing can have been launched
    for kw, match in ((dict(pano_width=1), "pano_width < 2"), (dict(pano_width=193, num_phi=0), "num_phi < 1"), (dict(pano_width=193, subpixel_bits=3), "subpixel_bits"),
                      (dict(pano_width=193), "ctx is null")):
        with pytest.raises(_lib.SsfmError, match="ssfm_pano_synthesize: " + match):
            pano.synthesize(None, s["R"], s["t"], s["intr"], frames, None, **kw)
    with pytest.raises(_lib.SsfmError, match="frame 2 is null"):
        pano.synthesize(None, s["R"], s["t"], s["intr"], [frames[0], frames[1], None] + list(frames[3:]), None, pano_width=193)
    with pytest.raises(_lib.SsfmError, match="flow of pair 6 is null"):
        pano.synthesize(None, s["R"], s["t"], s["intr"], frames, (list(flow[:6]) + [None], flow), pano_width=193)
    with pytest.raises(_lib.SsfmError, match="ctx is null"):                 # an open sweep has no pair 6: its flow entry is not looked at
        pano.synthesize(None, s["R"], s["t"], s["intr"], frames, (list(flow[:6]) + [None], list(flow[:6]) + [None]), pano_width=193, is_loop=0)
    with pytest.raises(_lib.SsfmError, match="ssfm_pano_plan: pano_width < 2"):
        pano.plan(s["R"], s["t"], s["intr"], 48, 37, 1)
    with pytest.raises(ValueError):
        pano.synthesize(None, s["R"], s["t"], s["intr"], frames[:6], None, pano_width=193)


def test_restatement_pixel_path_properties():
    """What the GPU comparisons rest on, checked on the restatement alone: bilinear at integer coordinates returns the pixel, outside taps are 0, a NaN coordinate
    samples 0, the 1/32 grid moves a coordinate, bytes are rounded half to even and saturated."""
    img = np.arange(2 * 3 * 4 * 3, dtype=np.float32).reshape(2, 3, 4, 3)
    x = np.array([[1.0, 3.0, -1.0, 3.5, np.nan, 2.0 ** 31]], np.float32).repeat(2, 0); y = np.array([[2.0, 0.0, 0.0, 1.0, 0.0, 0.0]], np.float32).repeat(2, 0)
    v = PR.bilinear(img, x, y, False)
    assert np.array_equal(v[0, 0], img[0, 2, 1]) and np.array_equal(v[1, 1], img[1, 0, 3]) and not v[:, 2].any() and not v[:, 4:].any()
    assert np.array_equal(v[0, 3], img[0, 1, 3] * np.float32(0.5))
    a = PR.bilinear(img, np.full((2, 1), 1.26, np.float32), np.full((2, 1), 0.51, np.float32), True)
    b = PR.bilinear(img, np.full((2, 1), 1.25, np.float32), np.full((2, 1), 0.5, np.float32), False)
    assert np.array_equal(a, b) and not np.array_equal(a, PR.bilinear(img, np.full((2, 1), 1.26, np.float32), np.full((2, 1), 0.51, np.float32), False))
    assert PR.to_byte(np.array([0.5, 1.5, 2.5, -3.0, 254.5, 255.5, 300.0, np.nan, np.inf], np.float32)).tolist() == [0, 2, 2, 0, 254, 255, 255, 0, 255]


def test_plan_levelling_and_file_readers_under_sanitizers(tmp_path):
    """tests/native/pano_host_check.cpp: the plan's `ok` shortcut against the all-rows rule, owner = highest ok pair, one thread = four threads, degenerate sizes;
    level_keyframes / compute_thetas / trim_loop of the shim; PPM and .flo round trips and truncated files.  ASan + UBSan, host code only."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "pano_host_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tests", "native", "pano_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    scratch = tmp_path / "files"; scratch.mkdir()
    run = subprocess.run([exe, str(scratch)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "PANO_HOST_CHECK ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr
