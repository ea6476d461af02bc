"""CPU side of the device track pass (ssfm_build_tracks_device): the restatement its GPU tests compare with (tests/_tracks_device_ref.py) against the host
bookkeeping (ssfm_build_tracks, merge = true) under the relation include/ssfm.h states; the exported symbols; the argument checks, which come before the
context is looked at and can therefore be made without one; the resources of the new kernels read from the built code object.  No kernel is launched here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _tracks_device_ref as REF
from spherical_sfm_amd import _lib, tracks
from spherical_sfm_amd._lib import c_double_p, c_i32_p, c_i64_p, c_u8_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIB = os.path.join(ROOT, "spherical_sfm_amd", "libssfm_hip.so")


def compare_with_host(ref, host, fptr):
    """the relation of the header: same partition, alive ids = components, same keys, equal pixels where a key holds one feature -> number of such keys"""
    H = REF.relabel_host(host, fptr)
    assert np.array_equal(ref["tracks"], H["tracks"])                        # canonical labels of equal partitions are equal arrays
    assert ref["num_points"] == H["num_points"]
    keys = REF.device_keys(ref)
    assert set(keys) == set(H["keys"]) == set(H["members"])
    single = [k for k, n in H["members"].items() if n == 1]
    for k in single:
        assert keys[k] == H["keys"][k]                                       # one subtraction on both sides: the same bits
    return len(single), len(keys)


@pytest.mark.parametrize("wrong_frac", [0.0, 0.05])
def test_restatement_against_host_tracks(wrong_frac):
    feats, ims = REF.scene(12, 200, 300, REF.chain_pairs(12, 3, extra=10, seed=1), wrong_frac=wrong_frac, seed=2)
    host = tracks.build_tracks(feats, ims, 500.0, 400.0, merge=True)
    flat = REF.flatten(feats, ims)
    ref = REF.components(*flat, 500.0, 400.0)
    single, nkeys = compare_with_host(ref, host, flat[0])
    if wrong_frac == 0.0:
        assert host["num_points"] > ref["num_points"] + 50                   # many tracks were started apart and merged later
        assert not ref["conflict"].any() and single == nkeys
    else:
        assert ref["conflict"].any() and single < nkeys                      # the conflicted keys are there, so the exemption is not vacuous
    assert (np.diff(ref["obs_cam"].astype(np.int64) * (1 << 32) + ref["obs_feat"]) > 0).all()      # ascending winning feature


def test_restatement_small_example():
    # frame 1 holds two features of one track: the smaller index wins the observation, the track is flagged; a self-match is a track of one feature
    fptr = np.array([0, 2, 4, 5], np.int32); fxy = np.arange(10, dtype=np.float64).reshape(5, 2)
    i0 = np.array([2, 0, 1, 0], np.int32); i1 = np.array([1, 1, 1, 0], np.int32); mptr = np.array([0, 1, 2, 2, 3], np.int32)
    f0 = np.array([0, 0, 1], np.int32); f1 = np.array([1, 0, 1], np.int32)
    r = REF.components(fptr, fxy, i0, i1, mptr, f0, f1, 1.0, 2.0)
    # edges: (4, 3), (0, 2), self (1, 1) -> components {0, 2}, {1}, {3, 4}
    assert r["tracks"].tolist() == [0, 1, 0, 2, 2] and r["num_points"] == 3 and r["conflict"].tolist() == [False, False, False]
    assert r["obs_cam"].tolist() == [0, 0, 1, 1, 2] and r["obs_pt"].tolist() == [0, 1, 0, 2, 2] and r["obs_feat"].tolist() == [0, 1, 0, 1, 0]
    assert r["obs_xy"].tolist() == [[-1.0, -1.0], [1.0, 1.0], [3.0, 3.0], [5.0, 5.0], [7.0, 7.0]]
    r = REF.components(fptr, fxy, np.array([1], np.int32), np.array([1], np.int32), np.array([0, 1], np.int32), np.array([1], np.int32), np.array([0], np.int32))
    assert r["tracks"].tolist() == [-1, -1, 0, 0, -1] and r["conflict"].tolist() == [True] and r["obs_feat"].tolist() == [0] and r["obs_cam"].tolist() == [1]


def test_new_symbols_are_exported():
    L = _lib.lib()
    for s in ("ssfm_build_tracks_device", "ssfm_tracks_last_kernel_ms"):
        assert hasattr(L, s) and s in _lib.DECLARED_SYMBOLS
    assert callable(tracks.build_tracks_device) and callable(tracks.build_tracks_device_flat) and callable(tracks.last_kernel_ms)
    assert L.ssfm_tracks_last_kernel_ms(None, None) == -1
    assert L.ssfm_version() == 100


def _call(fptr, i0, i1, mptr, f0=None, f1=None, K=None, S=None, skip=(), obs=True):
    """the C call without a context -> (rc, message)"""
    fptr = np.asarray(fptr, np.int32); i0 = np.asarray(i0, np.int32); i1 = np.asarray(i1, np.int32); mptr = np.asarray(mptr, np.int32)
    f0 = np.zeros(4, np.int32) if f0 is None else np.asarray(f0, np.int32); f1 = np.zeros(4, np.int32) if f1 is None else np.asarray(f1, np.int32)
    fxy = np.zeros((16, 2)); tr = np.zeros(16, np.int32); conf = np.zeros(16, np.uint8); npts = C.c_int32(0); nobs = C.c_int64(0)
    oc = np.zeros(16, np.int32); op = np.zeros(16, np.int32); of = np.zeros(16, np.int32); oxy = np.zeros((16, 2))
    a = dict(feat_ptr=fptr.ctypes.data_as(c_i32_p), feat_xy=fxy.ctypes.data_as(c_double_p), ms_index0=i0.ctypes.data_as(c_i32_p), ms_index1=i1.ctypes.data_as(c_i32_p),
             ms_ptr=mptr.ctypes.data_as(c_i32_p), m_f0=f0.ctypes.data_as(c_i32_p), m_f1=f1.ctypes.data_as(c_i32_p), tracks=tr.ctypes.data_as(c_i32_p),
             num_points=C.pointer(npts), conflict=conf.ctypes.data_as(c_u8_p), num_observations=C.pointer(nobs),
             obs_cam=oc.ctypes.data_as(c_i32_p) if obs else None, obs_pt=op.ctypes.data_as(c_i32_p) if obs else None,
             obs_feat=of.ctypes.data_as(c_i32_p) if obs else None, obs_xy=oxy.ctypes.data_as(c_double_p) if obs else None)
    for k in skip:
        a[k] = None
    L = _lib.lib()
    rc = L.ssfm_build_tracks_device(None, len(fptr) - 1 if K is None else K, a["feat_ptr"], a["feat_xy"], len(i0) if S is None else S, a["ms_index0"], a["ms_index1"],
                                    a["ms_ptr"], a["m_f0"], a["m_f1"], 0.0, 0.0, a["tracks"], C.cast(a["num_points"], c_i32_p) if a["num_points"] else None, a["conflict"],
                                    C.cast(a["num_observations"], c_i64_p) if a["num_observations"] else None, a["obs_cam"], a["obs_pt"], a["obs_feat"], a["obs_xy"])
    return rc, (L.ssfm_last_error(None) or b"").decode()


def test_argument_checks_refuse_before_the_context_is_looked_at():
    ok = dict(fptr=[0, 3, 5], i0=[0], i1=[1], mptr=[0, 2])
    msgs = []

    def refused(what, **kw):
        rc, msg = _call(**{**ok, **kw})
        assert rc == -1 and what in msg and msg.startswith("ssfm_build_tracks_device: "), (what, rc, msg)
        msgs.append(msg)

    for name in ("feat_ptr", "tracks", "num_points", "num_observations"):    # the order of include/ssfm.h
        refused("are required", skip=(name,))
    refused("together or not at all", skip=("obs_feat",))
    for name in ("ms_index0", "ms_index1", "ms_ptr"):
        refused("ms_index0, ms_index1 and ms_ptr are required", skip=(name,))
    refused("num_match_sets is >= 0", S=-1)
    refused("num_keyframes must be positive", K=0)
    refused("num_keyframes must be positive", K=-3)
    refused("feat_ptr[0] must be 0", fptr=[1, 3, 5])
    refused("feat_ptr must ascend", fptr=[0, 3, 2])
    refused("feat_xy is null", skip=("feat_xy",))
    refused("ms_ptr[0] must be 0", mptr=[1, 2])
    refused("ms_ptr must ascend", mptr=[0, -1])
    refused("m_f0 and m_f1 are required", skip=("m_f1",))
    for bad0, bad1 in (([2], [1]), ([0], [-1])):
        refused("frame index out of range", i0=bad0, i1=bad1)
    # an earlier refusal wins over a later one: num_keyframes before feat_ptr, feat_ptr before ms_ptr, ms_ptr before the frame indices
    refused("num_keyframes must be positive", K=0, fptr=[1, 3, 5])
    refused("feat_ptr must ascend", fptr=[0, 3, 2], mptr=[0, -1])
    refused("ms_ptr must ascend", mptr=[0, -1], i0=[7])
    refused("ctx is null")                                                   # everything in order: only now the missing context is noticed
    refused("ctx is null", obs=False)                                        # the four observation arrays NULL together: a counting call
    refused("ctx is null", S=0, skip=("ms_index0", "ms_index1", "ms_ptr", "m_f0", "m_f1"))      # no match sets: their arrays are not needed


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(KR.READELF)), reason="needs the built library and llvm-readelf")
def test_track_kernels_have_no_scratch():
    ks = {k["short"]: k for k in KR.kernels(LIB).values()}
    for want in ("k_tracks_init", "k_tracks_link", "k_tracks_roots", "k_tracks_scan_sums", "k_tracks_ids", "k_tracks_assign", "k_tracks_winners", "k_tracks_compact"):
        names = [n for n in ks if n.startswith(want) or ("::" + want) in n]
        assert names, (want, [n for n in ks if "tracks" in n])
        for n in names:
            k = ks[n]
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k
