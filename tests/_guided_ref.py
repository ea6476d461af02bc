"""Test helper: numpy restatement of guided matching (include/ssfm.h: ssfm_guided_match_pairs), written from the rule in the header, not from the device code.

  b_j = E u_j,  a_i = E^T v_i,  d = v_i . b_j,  den = b_j.x^2 + b_j.y^2 + a_i.x^2 + a_i.y^2;   cand(i, j)  <=>  d d < thr2 den          (fp64)
  per query i, among its candidates only: j1, j2 = nearest and second nearest train rows by the direct distance, lower j first on ties
  accepted iff  j1 exists  and  dist1 <= max_distance  and  (j2 absent  or  dist1 < ratio dist2 on the float distances, compared in double)
  m01[j1] = i, a later query overwrites; the list is (j, i) in ascending j

E is a (3, 3) numpy matrix with v^T E u = 0 (u: train / frame0, v: query / frame1)."""
import numpy as np

import _front_scene as FS


def sampson_parts(u, v, E):
    """-> (S (n1, n0) = d d, den (n1, n0)): cand = S < thr2 * den"""
    u = np.asarray(u, np.float64).reshape(-1, 3); v = np.asarray(v, np.float64).reshape(-1, 3); E = np.asarray(E, np.float64)
    b = u @ E.T                                                                      # b_j = E u_j
    a = v @ E                                                                        # a_i = E^T v_i
    d = v @ b.T
    den = (b[:, 0] ** 2 + b[:, 1] ** 2)[None, :] + (a[:, 0] ** 2 + a[:, 1] ** 2)[:, None]
    return d * d, den


def cand_mask(u, v, E, thr2):
    S, den = sampson_parts(u, v, E)
    with np.errstate(invalid="ignore", over="ignore"):
        return S < thr2 * den                                                        # NaN and 0 < 0 are False


def band_gap(S, thr2):
    """min |S / thr2 - 1| with S the Sampson values d d / den: how far the nearest entry is from the band's edge, relative"""
    S = np.asarray(S, np.float64)
    S = S[np.isfinite(S)]
    if S.size == 0 or not thr2 > 0:
        return np.inf
    return float(np.abs(S / thr2 - 1.0).min())


def sampson(u, v, E):
    S, den = sampson_parts(u, v, E)
    with np.errstate(invalid="ignore", divide="ignore"):
        return S / den


def knn2(train, u, query, v, E, thr2):
    """-> (nn (n1, 2) int32 [-1], dist (n1, 2) float32 [inf], cand_count (n1,) int32): the two nearest train rows among the candidates of every query"""
    t = np.asarray(train, np.float64); q = np.asarray(query, np.float64)
    q = q.reshape(-1, t.shape[1] if t.ndim == 2 and t.shape[0] else q.shape[-1]); t = t.reshape(-1, q.shape[1])
    n0, n1 = len(t), len(q)
    nn = np.full((n1, 2), -1, np.int32); d2 = np.full((n1, 2), np.inf)
    mask = cand_mask(u, v, E, thr2) if n0 and n1 else np.zeros((n1, n0), bool)
    for i in range(n1):
        js = np.flatnonzero(mask[i])
        if len(js) == 0:
            continue
        diff = q[i][None, :] - t[js]
        dd = (diff * diff).sum(1)
        order = np.argsort(dd, kind="stable")[:2]                                    # js ascends: a stable sort keeps the lower index on ties
        nn[i, :len(order)] = js[order]; d2[i, :len(order)] = dd[order]
    dist = np.sqrt(d2.astype(np.float32)).astype(np.float32)
    return nn, dist, mask.sum(1).astype(np.int32)


def guided_pair(train, u, query, v, E, thr2, ratio=0.75, max_distance=np.inf):
    """-> (idx0, idx1) int32: (j, i) sorted by j"""
    nn, dist, _ = knn2(train, u, query, v, E, thr2)
    m01 = {}
    for i in range(len(nn)):
        if nn[i, 0] < 0 or not dist[i, 0] <= np.float32(max_distance):
            continue
        if nn[i, 1] >= 0 and not float(dist[i, 0]) < ratio * float(dist[i, 1]):
            continue
        m01[int(nn[i, 0])] = i
    js = sorted(m01)
    return np.array(js, np.int32), np.array([m01[j] for j in js], np.int32)


def guided_triple_loop(train, u, query, v, E, thr2, ratio=0.75, max_distance=np.inf):
    """the same by plain loops (tiny inputs only): the check of the restatement itself"""
    t = np.asarray(train, np.float64); q = np.asarray(query, np.float64)
    u = np.asarray(u, np.float64).reshape(-1, 3); v = np.asarray(v, np.float64).reshape(-1, 3); E = np.asarray(E, np.float64)
    m01 = {}
    for i in range(len(q)):
        best = []                                                                    # (squared distance, train index) of the candidates
        for j in range(len(t)):
            b = [sum(E[r, c] * u[j, c] for c in range(3)) for r in range(3)]
            a = [sum(E[r, c] * v[i, r] for r in range(3)) for c in range(3)]
            d = sum(v[i, r] * b[r] for r in range(3))
            den = b[0] * b[0] + b[1] * b[1] + a[0] * a[0] + a[1] * a[1]
            if not d * d < thr2 * den:
                continue
            s = 0.0
            for k in range(t.shape[1]):
                s += (q[i, k] - t[j, k]) ** 2
            best.append((s, j))
        best.sort()
        if not best:
            continue
        d1 = np.sqrt(np.float32(best[0][0]))
        if not d1 <= np.float32(max_distance):
            continue
        if len(best) > 1 and not float(d1) < ratio * float(np.sqrt(np.float32(best[1][0]))):
            continue
        m01[best[0][1]] = i
    js = sorted(m01)
    return np.array(js, np.int32), np.array([m01[j] for j in js], np.int32)


def guided_pairs(descs_per_frame, rays_per_frame, pairs, Es, thr2, ratio=0.75, max_distance=np.inf):
    """-> (match_ptr [P+1], idx0, idx1) like ssfm_guided_match_pairs"""
    ptr = [0]; a0 = []; a1 = []
    for (f0, f1), E in zip(pairs, Es):
        j, i = guided_pair(descs_per_frame[f0], rays_per_frame[f0], descs_per_frame[f1], rays_per_frame[f1], E, thr2, ratio, max_distance)
        a0.append(j); a1.append(i); ptr.append(ptr[-1] + len(j))
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)
    return np.array(ptr, np.int32), cat(a0), cat(a1)


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------

def essential_of_step(step_deg, inward=False):
    """(E, R) of two cameras of _front_scene step_deg apart, camera 0 at angle 0, from the camera model itself: x_cam = R_i X + t with t = (0, 0, -1), so
    x1 = R x0 + (t - R t) with R = R_1 R_0^T, and E = [t - R t]x R."""
    from spherical_sfm_amd import synth
    R = synth.so3exp(np.array([0.0, step_deg * np.pi / 180, 0.0]))
    tz = np.array([0.0, 0.0, -1.0])
    t = tz - R @ tz
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R, R


def repeated_pair(seed, n=200, dim=128, rep=0.5, step_deg=4, noise_px=0.3):
    """Two cameras step_deg apart on the sphere see the same n points with noise_px of noise; a fraction `rep` of the points share their descriptor with one
    other point (pairs of twins), every observation carrying its own integer descriptor noise.  Features are shuffled in both frames.
    -> dict(train, u, query, v, E, R, truth): truth[i] = the train row of the point query i observes"""
    rng = np.random.default_rng(seed)
    ang1 = step_deg * np.pi / 180
    X, D = FS._world(rng, n, 0.5 * ang1, dim)
    nrep = int(rep * n) // 2 * 2
    D[1:nrep:2] = D[0:nrep:2]                                                        # twins: points 2 k and 2 k + 1 look alike
    xy0 = FS._project(X, 0.0, rng, noise_px); xy1 = FS._project(X, ang1, rng, noise_px)
    d0 = FS._noisy(D, rng); d1 = FS._noisy(D, rng)
    p0 = rng.permutation(n); p1 = rng.permutation(n)
    inv0 = np.empty(n, int); inv0[p0] = np.arange(n)
    E, R = essential_of_step(step_deg)
    return dict(train=d0[p0], u=FS.rays_of(xy0[p0]), query=d1[p1], v=FS.rays_of(xy1[p1]), E=E, R=R, truth=inv0[p1].astype(np.int32), repeated=(p1 < nrep))


THR2 = (2.0 / 600) ** 2
