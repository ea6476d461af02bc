"""ssfm_build_tracks_device on the GPU against its restatement (tests/_tracks_device_ref.py) and against the host bookkeeping (ssfm_build_tracks, merge = true)
under the relation include/ssfm.h states.  Everything here is integer work compared exactly; the pixels are one subtraction and compared exactly too."""
import ctypes as C

import numpy as np
import pytest

import _tracks_device_ref as REF
from spherical_sfm_amd import _lib, tracks

pytestmark = pytest.mark.gpu

CX, CY = 500.0, 400.0
FIELDS = ("tracks", "conflict", "obs_cam", "obs_pt", "obs_feat", "obs_xy")


def equal(a, b):
    return a["num_points"] == b["num_points"] and all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(a[k], b[k]) for k in FIELDS)


def blob(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in FIELDS) + np.int64(r["num_points"]).tobytes()


@pytest.fixture(scope="module")
def clean():
    feats, ims = REF.scene(12, 200, 300, REF.chain_pairs(12, 3, extra=10, seed=1), wrong_frac=0.0, seed=2)
    flat = REF.flatten(feats, ims)
    return dict(feats=feats, ims=ims, flat=flat, ref=REF.components(*flat, CX, CY), host=tracks.build_tracks(feats, ims, CX, CY, merge=True))


@pytest.fixture(scope="module")
def noisy():
    feats, ims = REF.scene(12, 200, 300, REF.chain_pairs(12, 3, extra=10, seed=1), wrong_frac=0.05, seed=2)
    flat = REF.flatten(feats, ims)
    return dict(feats=feats, ims=ims, flat=flat, ref=REF.components(*flat, CX, CY), host=tracks.build_tracks(feats, ims, CX, CY, merge=True))


def test_conflict_free_equals_restatement_and_host(gpu_ctx, clean):
    assert len(clean["ims"]) == 40
    got = tracks.build_tracks_device_flat(gpu_ctx, *clean["flat"], CX, CY)
    assert equal(got, clean["ref"]) and not got["conflict"].any()
    H = REF.relabel_host(clean["host"], clean["flat"][0])
    assert clean["host"]["num_points"] > H["num_points"]                     # the host issued ids that merges consumed
    assert np.array_equal(got["tracks"], H["tracks"]) and got["num_points"] == H["num_points"]
    assert REF.device_keys(got) == H["keys"] and len(H["keys"]) == len(got["obs_cam"])      # keys and pixels, exactly
    lists = tracks.build_tracks_device(gpu_ctx, clean["feats"], clean["ims"], CX, CY)     # the list form: the same call on the same arrays
    assert np.array_equal(np.concatenate(lists["tracks"]), got["tracks"]) and np.array_equal(lists["obs_xy"], got["obs_xy"])


def test_conflicted_equals_restatement(gpu_ctx, noisy):
    got = tracks.build_tracks_device_flat(gpu_ctx, *noisy["flat"], CX, CY)
    assert equal(got, noisy["ref"])
    assert got["conflict"].any()                                              # the case is not vacuous
    H = REF.relabel_host(noisy["host"], noisy["flat"][0])
    assert np.array_equal(got["tracks"], H["tracks"]) and got["num_points"] == H["num_points"]
    keys = REF.device_keys(got)
    assert set(keys) == set(H["keys"])
    single = [k for k, n in H["members"].items() if n == 1]
    assert 0 < len(single) < len(keys) and all(keys[k] == H["keys"][k] for k in single)
    assert all(got["conflict"][k[1]] for k, n in H["members"].items() if n > 1)


def test_order_independence(gpu_ctx, noisy):
    fptr, fxy, i0, i1, mptr, f0, f1 = noisy["flat"]
    base = tracks.build_tracks_device_flat(gpu_ctx, fptr, fxy, i0, i1, mptr, f0, f1, CX, CY)
    again = tracks.build_tracks_device_flat(gpu_ctx, fptr, fxy, i0, i1, mptr, f0, f1, CX, CY)
    assert blob(base) == blob(again)
    rng = np.random.default_rng(7)
    order = rng.permutation(len(i0)).tolist()
    order.insert(5, order[20])                                               # one set twice
    sets = []
    for s in order:
        m = np.arange(mptr[s], mptr[s + 1]); m = m[rng.permutation(len(m))]  # the matches inside the set permuted
        sets.append((int(i0[s]), int(i1[s]), list(zip(f0[m].tolist(), f1[m].tolist()))))
    p = REF.flatten(noisy["feats"], sets)
    assert len(p[2]) == len(i0) + 1 and not np.array_equal(p[5][:len(f0)], f0)
    assert blob(tracks.build_tracks_device_flat(gpu_ctx, *p, CX, CY)) == blob(base)


def test_deep_trees(gpu_ctx):
    K = 1500
    feats = [np.arange(6, dtype=np.float64).reshape(3, 2) + 10.0 * k for k in range(K)]
    ims = [(k, k + 1, [(0, 0), (1, 1), (2, 2)]) for k in range(K - 2, -1, -1)]               # descending k: the longest chain the hooking can build
    got = tracks.build_tracks_device_flat(gpu_ctx, *REF.flatten(feats, ims))
    assert got["num_points"] == 3 and not got["conflict"].any()
    assert np.array_equal(got["tracks"], np.tile(np.arange(3, dtype=np.int32), K))
    assert np.array_equal(got["obs_cam"], np.repeat(np.arange(K, dtype=np.int32), 3)) and np.array_equal(got["obs_pt"], got["tracks"])
    assert np.array_equal(got["obs_feat"], got["tracks"]) and np.array_equal(got["obs_xy"], np.concatenate(feats))
    assert (np.bincount(got["obs_pt"]) == K).all()


def test_scan_boundaries(gpu_ctx):
    K, n = 35, 2003                                                          # 70 105 features: no multiple of 64, 256 or 1024, 274 scan blocks
    feats, ims = REF.scene(K, n, 3000, REF.chain_pairs(K, 2), wrong_frac=0.0, seed=11, max_matches=150)
    flat = REF.flatten(feats, ims)
    assert flat[0][-1] == 70105
    got = tracks.build_tracks_device_flat(gpu_ctx, *flat, CX, CY)
    ref = REF.components(*flat, CX, CY)
    assert equal(got, ref) and got["num_points"] > 1000 and (got["tracks"] < 0).any()
    assert (np.flatnonzero(got["tracks"] >= 0) // 256).max() > 256            # ids and observations past one round of the scan over the block sums


def test_edges(gpu_ctx):
    feats = [np.arange(8, dtype=np.float64).reshape(4, 2), np.zeros((0, 2)), np.arange(6, dtype=np.float64).reshape(3, 2) + 100.0]
    fptr = np.array([0, 4, 4, 7], np.int32); fxy = np.concatenate(feats)
    none = np.zeros(0, np.int32)
    r = tracks.build_tracks_device_flat(gpu_ctx, fptr, fxy, none, none, np.zeros(1, np.int32), none, none)          # zero match sets
    assert r["tracks"].tolist() == [-1] * 7 and r["num_points"] == 0 and len(r["obs_cam"]) == 0 and len(r["conflict"]) == 0
    r = tracks.build_tracks_device_flat(gpu_ctx, fptr, fxy, [0, 1], [2, 2], [0, 0, 0], none, none)                  # empty sets only
    assert r["tracks"].tolist() == [-1] * 7 and r["num_points"] == 0 and r["num_observations"] == 0
    # an empty set, a frame without features, a set inside one frame (flagged), a self-match (a track of one feature)
    i0 = [0, 1, 2, 0, 0]; i1 = [2, 2, 2, 0, 2]; mptr = [0, 0, 0, 1, 2, 3]; f0 = [0, 3, 1]; f1 = [2, 3, 1]
    r = tracks.build_tracks_device_flat(gpu_ctx, fptr, fxy, i0, i1, mptr, f0, f1, 1.0, 2.0)
    ref = REF.components(fptr, fxy, np.array(i0), np.array(i1), np.array(mptr), np.array(f0), np.array(f1), 1.0, 2.0)
    assert equal(r, ref)
    assert r["tracks"].tolist() == [-1, 0, -1, 1, 2, 0, 2] and r["conflict"].tolist() == [False, False, True]
    assert r["obs_cam"].tolist() == [0, 0, 2, 2] and r["obs_feat"].tolist() == [1, 3, 0, 1] and r["obs_pt"].tolist() == [0, 1, 2, 0]
    c = tracks.build_tracks_device_flat(gpu_ctx, fptr, fxy, i0, i1, mptr, f0, f1, observations=False)              # counts only
    assert c["num_observations"] == 4 and c["num_points"] == 3 and c["obs_cam"] is None and np.array_equal(c["tracks"], r["tracks"])
    assert c["conflict"].tolist() == [False, False, True]


def test_invalid_feature_index_is_refused_and_the_context_survives(gpu_ctx, clean):
    fptr, fxy, i0, i1, mptr, f0, f1 = clean["flat"]
    n1 = int(fptr[i1[3] + 1] - fptr[i1[3]])
    for bad in (n1, -1):
        g1 = f1.copy(); g1[mptr[3]] = bad                                    # one past its frame / negative
        with pytest.raises(_lib.SsfmError, match="ssfm_build_tracks_device: feature index out of range"):
            tracks.build_tracks_device_flat(gpu_ctx, fptr, fxy, i0, i1, mptr, f0, g1, CX, CY)
    assert equal(tracks.build_tracks_device_flat(gpu_ctx, fptr, fxy, i0, i1, mptr, f0, f1, CX, CY), clean["ref"])


def test_kernel_timer(gpu_ctx, clean):
    tracks.build_tracks_device_flat(gpu_ctx, *clean["flat"], CX, CY)
    assert tracks.last_kernel_ms(gpu_ctx) > 0.0
    ms = C.c_double(5.0)
    assert _lib.lib().ssfm_tracks_last_kernel_ms(None, C.byref(ms)) == -1
