"""Test helper: numpy restatement of match / match_exhaustive (reference examples/spherical_sfm_tools.cpp:235-251, :575-600), written from those
lines and from the documented behaviour of cv::BFMatcher (NORM_L2, knnMatch(query, train, 2)), not from the device code.

  train = descriptors of features0, query = descriptors of features1                                    (:241-242)
  per query i, ascending: the two nearest train rows (j1, j2) by L2 distance, dist a float               (knnMatch k = 2)
  if dist1 < ratio * dist2 (float * double -> compared in double):  m01[j1] = i                          (:246-249)
  m01 is a std::map: a later query overwrites, the result is sorted by j                                 (header :20)

Ranking is by the DIRECT float64 distances sum (q - t)^2.  For large frames the float64 product form only preselects SHORTLIST candidates per query
(its error, ~1e-15 relative to |q|^2 + |t|^2, cannot push a true top-2 row out of the best SHORTLIST); the rank among them, the distances and the
test all come from the direct form.  Equal distances rank the lower train index first.  A train set with fewer than two rows gives no matches (the
reference would index past matches[i]); both choices are the ones include/ssfm.h documents."""
import numpy as np

SHORTLIST = 8


def knn2(train, query):
    """-> (nn (n1, 2) int32 [-1: no such row], d2 (n1, 2) float64 squared direct distances [inf], dist (n1, 2) float32 = sqrtf(float(d2)))"""
    t = np.asarray(train, np.float64).reshape(-1, np.asarray(query).shape[-1]); q = np.asarray(query, np.float64).reshape(-1, t.shape[1])
    n0, n1 = len(t), len(q)
    nn = np.full((n1, 2), -1, np.int32); d2 = np.full((n1, 2), np.inf)
    if n0 and n1:
        k = min(SHORTLIST, n0)
        tt = (t * t).sum(1)
        for a in range(0, n1, 512):
            qa = q[a:a + 512]
            if n0 > k:
                g = tt[None, :] - 2.0 * (qa @ t.T)                                  # |q|^2 is common to a row
                cand = np.sort(np.argpartition(g, k - 1, axis=1)[:, :k], axis=1)     # ascending index: a stable sort then keeps the lower index on ties
            else:
                cand = np.tile(np.arange(n0), (len(qa), 1))
            diff = qa[:, None, :] - t[cand]                                          # direct form on the shortlist
            dd = (diff * diff).sum(2)
            order = np.argsort(dd, axis=1, kind="stable")[:, :2]
            rows = np.arange(len(qa))[:, None]
            m = order.shape[1]
            nn[a:a + 512, :m] = cand[rows, order]; d2[a:a + 512, :m] = dd[rows, order]
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(d2.astype(np.float32)).astype(np.float32)                     # the reference's distance is a float: sqrtf of a float sum
    return nn, d2, dist


def ratio_pass(dist, nn, ratio):
    """the test of :246 on float distances, compared in double; needs a second neighbour"""
    return (nn[:, 1] >= 0) & (dist[:, 0].astype(np.float64) < ratio * dist[:, 1].astype(np.float64))


def match_pair(train, query, ratio=0.75):
    """-> (idx0, idx1) int32: the std::map m01 as (j, i) sorted by j"""
    nn, _, dist = knn2(train, query)
    ok = ratio_pass(dist, nn, ratio)
    m01 = {}
    for i in range(len(nn)):                                                         # query order: a later query overwrites (std::map operator[])
        if ok[i]:
            m01[int(nn[i, 0])] = i
    js = sorted(m01)
    return np.array(js, np.int32), np.array([m01[j] for j in js], np.int32)


def ambiguous(d2, ratio, tol=1e-5):
    """queries whose ratio test is decided within tol: |d1 - ratio d2| <= tol d2 on the float64 distances"""
    d = np.sqrt(d2)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d[:, 1]) & (np.abs(d[:, 0] - ratio * d[:, 1]) <= tol * d[:, 1])


def match_pairs(descs_per_frame, pairs, ratio=0.75):
    """-> (match_ptr [P+1], idx0, idx1) like ssfm_match_pairs; pair (f0, f1): train = frame f0, query = frame f1"""
    ptr = [0]; a0 = []; a1 = []
    for f0, f1 in pairs:
        j, i = match_pair(descs_per_frame[f0], descs_per_frame[f1], ratio)
        a0.append(j); a1.append(i); ptr.append(ptr[-1] + len(j))
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)
    return np.array(ptr, np.int32), cat(a0), cat(a1)


def exhaustive_pairs(num_frames):
    """:577-586: index0 < index1, nested"""
    return [(a, b) for a in range(num_frames) for b in range(a + 1, num_frames)]


def match_triple_loop(train, query, ratio=0.75):
    """the same by plain loops (tiny inputs only): the check of the restatement itself"""
    t = np.asarray(train, np.float64); q = np.asarray(query, np.float64)
    m01 = {}
    if len(t) < 2:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    for i in range(len(q)):
        best = []                                                                   # (squared distance, train index), ascending
        for j in range(len(t)):
            s = 0.0
            for k in range(t.shape[1]):
                s += (q[i, k] - t[j, k]) ** 2
            best.append((s, j))
        best.sort()
        d1 = np.sqrt(np.float32(best[0][0])); d2 = np.sqrt(np.float32(best[1][0]))
        if float(d1) < ratio * float(d2):
            m01[best[0][1]] = i
    js = sorted(m01)
    return np.array(js, np.int32), np.array([m01[j] for j in js], np.int32)


# ---- generators -----------------------------------------------------------------------------------------------------------------------------

def world_pool(num, dim=128, seed=0):
    """SIFT-like world features: non-negative, a few strong bins"""
    rng = np.random.default_rng(seed)
    return np.abs(rng.standard_normal((num, dim))) ** 1.5


def integer_frame(pool, n, seed, span=None):
    """A frame of n descriptors as OpenCV's SIFT stores them (floats holding integers 0..255): a random subset of the first `span` pool features (default
    2 n: two frames of one size share about half), each with its own noise level, L2-normalised to 512, rounded, clipped."""
    rng = np.random.default_rng(seed)
    span = min(len(pool), max(2 * n, 4) if span is None else span)
    ids = rng.choice(span, n, replace=False) if n else np.zeros(0, int)
    level = rng.uniform(0.02, 0.6, (n, 1))
    v = np.maximum(pool[ids] * (1.0 + level * rng.standard_normal((n, pool.shape[1]))), 0.0)
    v = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12) * 512.0
    return np.clip(np.rint(v), 0, 255).astype(np.float32), ids


def float_frame(pool, n, seed, span=None):
    """unit-normalised, non-integer descriptors of the same construction"""
    rng = np.random.default_rng(seed)
    span = min(len(pool), max(2 * n, 4) if span is None else span)
    ids = rng.choice(span, n, replace=False) if n else np.zeros(0, int)
    level = rng.uniform(0.02, 0.6, (n, 1))
    v = np.maximum(pool[ids] * (1.0 + level * rng.standard_normal((n, pool.shape[1]))), 0.0)
    v = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    return v.astype(np.float32), ids
