"""ssfm_anms_batch on the GPU against the literal restatement of adaptiveNonMaximalSuppresion (tests/_anms_ref.py).  The contract is exact -- float differences,
double sums of exact products, one correctly rounded square root, integer counts -- so every comparison is array_equal: keep lists and the bit patterns of the
radii.  Sizes walk the edges of the kernel's shapes: the wave (64), the workgroup of keypoints i (256), the LDS tile of keypoints j (1024), more than one tile
(2500), and the j split forced at a small size."""
import os
import struct
import subprocess

import numpy as np
import pytest

from spherical_sfm_amd import _lib, features, pairwise

import _anms_ref as AR
import _front_scene as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2500]


def _keeps(n):
    return sorted({0, 1, n // 4, max(n - 1, 0), n, n + 1})


def _check(ctx, frames, keeps, **kw):
    """frames: list of (xy, response, keep, radius) from AR.reference; one device call for all of them"""
    got, rad = features.anms(ctx, [f[0] for f in frames], [f[1] for f in frames], keeps, return_radius=True, **kw)
    assert len(got) == len(frames)
    for f, g, rr, k in zip(frames, got, rad, keeps):
        assert g.dtype == np.int32 and rr.dtype == np.float64
        assert np.array_equal(g, f[2]), (len(f[1]), k)
        assert np.array_equal(rr.view(np.uint64), f[3].view(np.uint64)), (len(f[1]), k)
    return got, rad


@pytest.mark.parametrize("n", SIZES)
def test_keep_lists_and_radii_bit_for_bit(gpu_ctx, n):
    """SIFT-like input, every num_to_keep of {0, 1, n//4, n-1, n, n+1} as one frame of one batched call (n+1: returned unchanged; n: everything, sorted)."""
    keeps = _keeps(n)
    frames = [AR.reference("sift", n, 100 + n, k) for k in keeps]
    got, _ = _check(gpu_ctx, frames, keeps)
    for g, k in zip(got, keeps):
        assert len(g) >= min(n, k + 1)
    if n >= 255:
        # the guard on the input: the same restatement with the subtraction in double gives another radius somewhere, so a kernel that subtracted in
        # double (or squared in float) cannot pass above
        xy, r, _, rad = frames[2]
        assert (AR.anms_literal(xy, r, keeps[2], sub_in_double=True)[1] != rad).any()


def test_ragged_batch(gpu_ctx):
    sizes = [0, 1, 5, 300, 257, 1027, 64]
    keeps = [0, 1, 9, 75, 257, 200, 16]                # frame 2 is below its target (unchanged), frame 4 equal to it (everything, sorted)
    frames = [AR.reference("sift", n, 200 + i, k) for i, (n, k) in enumerate(zip(sizes, keeps))]
    got, rad = _check(gpu_ctx, frames, keeps)
    assert len(got[0]) == 0 and np.array_equal(got[2], np.arange(5)) and (rad[2] == AR.DBL_MAX).all() and len(got[4]) == 257
    assert features.last_kernel_ms(gpu_ctx) > 0.0
    assert features.anms(gpu_ctx, [], [], 10) == []                                      # num_frames = 0
    assert [len(k) for k in features.anms(gpu_ctx, [np.zeros((0, 2))] * 2, [np.zeros(0)] * 2, 10)] == [0, 0]


def test_ties(gpu_ctx):
    """Integer grid 40 x 30, responses k/64, duplicated points: radii tie, so more than num_to_keep + 1 survive; equal responses come out by index."""
    frames = [AR.reference("grid", 257, 4, 64), AR.reference("grid", 257, 4, 0), AR.reference("grid", 1500, 5, 300)]
    got, rad = _check(gpu_ctx, frames, [64, 0, 300])
    assert len(got[0]) > 64 + 1 and (rad[0] == 0.0).any()
    r = frames[0][1]; g = got[0]
    assert all(r[a] > r[b] or (r[a] == r[b] and a < b) for a, b in zip(g[:-1], g[1:])) and (r[g[:-1]] == r[g[1:]]).any()


def test_negative_and_zero_responses(gpu_ctx):
    frames = [AR.reference("signed", 200, 5, 50), AR.reference("signed", 700, 6, 0), AR.reference("signed", 33, 7, 33)]
    assert all((f[1] < 0).any() and (f[1] == 0).any() for f in frames)
    _check(gpu_ctx, frames, [50, 0, 33])


def test_forced_j_split_equals_the_unsplit_call(gpu_ctx):
    """force_j_chunks 2, 3, 7 at n = 700 (chunks of 350, 234, 100: no multiple of anything): the atomics combine to the bits of the one-chunk call, and twice."""
    frames = [AR.reference("sift", 700, 300, 175), AR.reference("grid", 700, 301, 100), AR.reference("signed", 700, 302, 699)]
    keeps = [175, 100, 699]
    base = _check(gpu_ctx, frames, keeps, force_j_chunks=1)
    for chunks in (2, 3, 7):
        a = _check(gpu_ctx, frames, keeps, force_j_chunks=chunks)
        b = _check(gpu_ctx, frames, keeps, force_j_chunks=chunks)
        for x, y in ((a, base), (b, a)):
            assert all(np.array_equal(p, q) for p, q in zip(x[0], y[0])) and all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(x[1], y[1]))
    _check(gpu_ctx, frames, keeps)                                                       # the planner's own cut: three small frames do not fill the device


def test_refusals_leave_the_library_usable(gpu_ctx):
    xy, r, keep, rad = AR.reference("sift", 257, 357, 64)
    bad = r.copy(); bad[100] = np.nan
    with pytest.raises(_lib.SsfmError, match="ssfm_anms_batch: NaN response"):
        features.anms(gpu_ctx, [xy], [bad], 64)
    with pytest.raises(_lib.SsfmError, match="ssfm_anms_batch: num_to_keep is negative"):
        features.anms(gpu_ctx, [xy], [r], -1)
    with pytest.raises(_lib.SsfmError, match="ssfm_anms_batch: kp_ptr is not ascending"):
        features.anms_flat(gpu_ctx, np.array([0, 257, 100], np.int32), np.concatenate([xy, xy]), np.concatenate([r, r]), [3, 3])
    _check(gpu_ctx, [(xy, r, keep, rad)], [64])


def test_select_feeds_the_pairwise_front_end(gpu_ctx):
    """features.select on four frames with descriptors -> pairwise.pairwise_from_features, against the same gather done in numpy with the restatement's keep lists."""
    frames = S.arc_frames((260, 300, 280, 40), dim=128, seed=11)
    rng = np.random.default_rng(12)
    resp = [(rng.uniform(0, 1, len(f[0])) ** 3 * 0.1).astype(np.float32) for f in frames]
    existing = [0, 100, 0, 250]; target = 250                                            # frame 3: ntokeep 0, skipped; frame 1 keeps 150 of 300
    ptr, descs, xy, keep = features.select(gpu_ctx, [f[0] for f in frames], resp, [f[1] for f in frames], existing=existing, target=target)
    want = [AR.anms_literal(f[0], r, target - e)[0] if target - e > 0 else np.zeros(0, np.int32) for f, r, e in zip(frames, resp, existing)]
    assert all(np.array_equal(a, b) for a, b in zip(keep, want)) and len(keep[3]) == 0 and len(keep[1]) >= 151 and len(keep[0]) >= 251
    hxy = np.concatenate([f[0].astype(np.float32)[k] for f, k in zip(frames, want)]); hd = np.concatenate([f[1][k] for f, k in zip(frames, want)])
    hptr = np.zeros(5, np.int32); hptr[1:] = np.cumsum([len(k) for k in want])
    assert np.array_equal(ptr, hptr) and np.array_equal(xy, hxy) and np.array_equal(descs, hd) and xy.dtype == np.float32 and descs.dtype == np.float32
    pairs = [(0, 1), (0, 2), (1, 2), (2, 3)]
    a = pairwise.pairwise_from_features(gpu_ctx, descs, S.rays_of(xy), ptr, pairs)
    b = pairwise.pairwise_from_features(gpu_ctx, hd, S.rays_of(hxy), hptr, pairs)
    assert len(a.accepted_pair) >= 2
    for name in ("accepted_pair", "R", "num_inliers", "inl_ptr", "inl_idx0", "inl_idx1", "match_count"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_cpp_mirror_prints_the_python_keep_lists(gpu_ctx, tmp_path):
    exe = os.path.join(ROOT, "spherical_sfm_amd", "demo_anms")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    sizes = [0, 5, 300, 257, 600]; keeps = [3, 9, 75, 257, 0]; existing = [0, 4000, 3925, 3990, 4001]
    frames = [AR.reference("sift" if i != 3 else "grid", n, 400 + i, k) for i, (n, k) in enumerate(zip(sizes, keeps))]
    path = str(tmp_path / "kp.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(frames)))
        for (xy, r, _, _), k, e in zip(frames, keeps, existing):
            f.write(struct.pack("<iii", len(r), k, e))
            f.write(np.concatenate([xy, r[:, None]], axis=1).astype("<f4").tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert "DEMO_ANMS_RESULT frames=5 single_equals_batched=1" in lines
    py = features.anms(gpu_ctx, [f[0] for f in frames], [f[1] for f in frames], keeps)
    for i, (fr, g) in enumerate(zip(frames, py)):
        assert np.array_equal(g, fr[2])
        assert "ANMS_FRAME %d %d" % (i, len(g)) + "".join(" %d" % v for v in g) in lines
    # select_keypoints: ntokeep = max(0, 4000 - existing); 0 selects nothing, otherwise the survivors' points are appended
    sel = features.select(gpu_ctx, [f[0] for f in frames], [f[1] for f in frames], None, existing=existing, target=4000)[3]
    assert [len(k) for k in sel][1] == 0 and len(sel[4]) == 0 and len(sel[2]) >= 76 and len(sel[3]) >= 11
    for i, k in enumerate(sel):
        assert "ANMS_SELECT %d %d %d %d" % (i, existing[i], existing[i] + len(k), len(k)) + "".join(" %d" % v for v in k) in lines
