"""Test helper: adaptiveNonMaximalSuppresion (examples/spherical_sfm_tools.cpp:76-123) restated literally in numpy -- a STABLE sort by response descending
(the reference's std::sort leaves the order among equal responses open; this project fixes it by original index), then for every i the loop over the j before it
that stops at the first response_j <= thr_i, radii in float-then-double arithmetic, the decision radius from the radii sorted descending, the keep list in sorted
order.  The reference of tests/test_anms_gpu.py and tests/test_anms_cpu.py; also the sort-free set form of the contract (include/ssfm.h) and the input generators.

Two places are defined where the reference is not: n == num_to_keep (it reads radiiSorted[n]) returns everything in sorted order, and n < num_to_keep returns
the input unchanged with radii DBL_MAX (the reference computes none)."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
COEFF = np.float32(1.11)


def _dist(xi, yi, xj, yj, sub_in_double=False):
    """cv::norm(pt_i - pt_j): the subtraction in float, then sqrt((double)dx*dx + (double)dy*dy).  sub_in_double: the WRONG recipe, for the input guard."""
    if sub_in_double:
        dx = np.float64(xi) - xj.astype(np.float64); dy = np.float64(yi) - yj.astype(np.float64)
    else:
        dx = (np.float32(xi) - xj).astype(np.float64); dy = (np.float32(yi) - yj).astype(np.float64)
    return np.sqrt(dx * dx + dy * dy)


def anms_literal(xy, response, num_to_keep, sub_in_double=False):
    """-> (keep: original indices in sorted order, radius: per INPUT keypoint)"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2); r = np.asarray(response, np.float32).reshape(-1)
    n = len(r)
    if n < num_to_keep:
        return np.arange(n, dtype=np.int32), np.full(n, DBL_MAX)
    order = np.argsort(-r.astype(np.float64), kind="stable")               # float -> double is exact and keeps the order; -0.0 and 0.0 stay equal
    xs, ys, rs = xy[order, 0], xy[order, 1], r[order]
    radii = np.full(n, DBL_MAX)
    for i in range(n):
        thr = np.float32(rs[i] * COEFF)
        fail = np.flatnonzero(~(rs[:i] > thr))                               # `j < i && response_j > thr`: the loop ends at the first j that fails
        m = fail[0] if len(fail) else i
        if m > 0:
            d = _dist(xs[i], ys[i], xs[:m], ys[:m], sub_in_double)
            d = d[d == d]                                                    # std::min(radius, NaN) keeps radius
            if len(d):
                radii[i] = min(DBL_MAX, d.min())
    if num_to_keep < n:
        decision = np.sort(radii)[::-1][num_to_keep]
    else:
        decision = 0.0
    kept = np.flatnonzero(radii >= decision)
    rad_in = np.empty(n); rad_in[order] = radii
    return order[kept].astype(np.int32), rad_in


def anms_set_form(xy, response, num_to_keep):
    """The sort-free form of include/ssfm.h: precedes(j, i), radius as a minimum over a set, rank as a count."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2); r = np.asarray(response, np.float32).reshape(-1)
    n = len(r)
    if n < num_to_keep:
        return np.arange(n, dtype=np.int32), np.full(n, DBL_MAX)
    idx = np.arange(n)
    radius = np.full(n, DBL_MAX); rank = np.zeros(n, np.int64)
    for i in range(n):
        pre = (r > r[i]) | ((r == r[i]) & (idx < i))
        rank[i] = pre.sum()
        sel = pre & (r > np.float32(r[i] * COEFF))
        if sel.any():
            dx = (xy[i, 0] - xy[sel, 0]).astype(np.float64); dy = (xy[i, 1] - xy[sel, 1]).astype(np.float64)
            d2 = dx * dx + dy * dy
            d2 = d2[d2 < np.inf]
            if len(d2):
                radius[i] = np.sqrt(d2.min())
    assert np.array_equal(np.sort(rank), idx)
    decision = np.sort(radius)[::-1][num_to_keep] if num_to_keep < n else 0.0
    keep = np.flatnonzero(radius >= decision)
    return keep[np.argsort(rank[keep])].astype(np.int32), radius


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------

def sift_like(n, seed):
    """x in [0, 1920), y in [0, 1080), response = u^3 * 0.1: many weak keypoints, few strong ones"""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(0, 1920, n), rng.uniform(0, 1080, n)], axis=1).astype(np.float32)
    return xy, (rng.uniform(0, 1, n) ** 3 * 0.1).astype(np.float32)


def tied_grid(n, seed, dup=8):
    """integer coordinates on a 40 x 30 grid, responses k/64: heavily tied responses and radii; the last `dup` points repeat earlier positions (radius 0 candidates)"""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.integers(0, 40, n), rng.integers(0, 30, n)], axis=1).astype(np.float32)
    if dup and n > 2 * dup:
        xy[n - dup:] = xy[:dup]
    return xy, (rng.integers(0, 64, n) / 64.0).astype(np.float32)


def signed(n, seed):
    """responses that are multiples of 1/8 in [-0.75, 0.75], zeros and negatives included"""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], axis=1).astype(np.float32)
    return xy, (rng.integers(-6, 7, n) / 8.0).astype(np.float32)


_CACHE = {}


def reference(kind, n, seed, num_to_keep):
    """(xy, response, keep, radius) of one generated input, computed once per session and handed out read-only"""
    key = (kind, n, seed, num_to_keep)
    if key not in _CACHE:
        xy, r = {"sift": sift_like, "grid": tied_grid, "signed": signed}[kind](n, seed)
        keep, rad = anms_literal(xy, r, num_to_keep)
        for a in (xy, r, keep, rad):
            a.setflags(write=False)
        _CACHE[key] = (xy, r, keep, rad)
    return _CACHE[key]
