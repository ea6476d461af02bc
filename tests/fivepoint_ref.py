"""Test-side restatement of the general (five-point) relative-pose path, numpy only, written from the mathematics and from the reference's
control flow -- not from the kernel, which reaches the same solutions another way (a degree-10 polynomial in one coordinate, bracketed roots).

  nullspace            np.linalg.svd of the 5x9 system [u_i v_j]
  cubics               det E = 0 and 2 E E^T E - tr(E E^T) E = 0 for E = x E1 + y E2 + z E3 + E4, by polynomial arithmetic
  solve                Gauss-Jordan on the ten cubic monomials -> the 10x10 action matrix of multiplication by x -> np.linalg.eig; a solution
                       is kept where |imag(eigenvalue)| <= 1e-9 (1 + |real|), then polished by Newton steps on the ten cubics
  residual             FivePointEstimator::EvaluateModelOnPoint: line = E (u / u2), (v . line)^2 / (line0^2 + line1^2)
  decompose / pose     DecomposeEssentialMatrix + the four-way cheirality vote of PoseFromEssentialMatrix, with the candidate order made
                       independent of the SVD routine (include/ssfm.h says how)
  replay               RansacLib's LocallyOptimizedMSAC::EstimateModel for a minimal sample of five over an estimator whose NonMinimalSolver
                       returns 0 and whose LeastSquares is empty, then estimate_pairwise_five_point's tail; both std::mt19937 streams come from
                       oracle.mt19937_draws (libstdc++'s engine and uniform_int_distribution)
"""
import numpy as np

DEG3 = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
LOW = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def nullspace(u5, v5):
    """(9, 4) orthonormal basis of the right nullspace of the rows [u0v0 u0v1 u0v2 u1v0 ... u2v2]"""
    A = np.einsum("ni,nj->nij", np.asarray(u5, float), np.asarray(v5, float)).reshape(5, 9)
    return np.linalg.svd(A)[2][5:].T


def _mul_lin(P, c):
    """polynomial P[ex, ey, ez] (degree <= 2) times the linear form c = (cx, cy, cz, c1)"""
    out = c[3] * P
    out[1:] += c[0] * P[:-1]; out[:, 1:] += c[1] * P[:, :-1]; out[:, :, 1:] += c[2] * P[:, :, :-1]
    return out


def _lin(c):
    P = np.zeros((4, 4, 4)); P[1, 0, 0], P[0, 1, 0], P[0, 0, 1], P[0, 0, 0] = c
    return P


def cubics(B):
    """the ten cubic constraints as polynomials [10, 4, 4, 4] in (x, y, z); E(r, c) = (B (x, y, z, 1))[r + 3c]"""
    e = lambda r, c: B[r + 3 * c]
    L = [[_lin(e(r, c)) for c in range(3)] for r in range(3)]
    out = []
    det = 0
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        det = det + _mul_lin(_mul_lin(L[1][j], e(2, k)) - _mul_lin(L[1][k], e(2, j)), e(0, i))
    out.append(det)
    EEt = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3): EEt[i][j] = EEt[j][i] = sum(_mul_lin(L[i][k], e(j, k)) for k in range(3))
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    Lam = [[2.0 * EEt[i][k] - (tr if i == k else 0.0) for k in range(3)] for i in range(3)]
    for i in range(3):
        for j in range(3):
            out.append(sum(_mul_lin(Lam[i][k], e(k, j)) for k in range(3)))
    return np.array(out)


def eval_cubics(C, x, y, z):
    px, py, pz = x ** np.arange(4), y ** np.arange(4), z ** np.arange(4)
    return np.einsum("kabc,a,b,c->k", C, px, py, pz)


def _monomials(s):
    px, py, pz = s[0] ** np.arange(4), s[1] ** np.arange(4), s[2] ** np.arange(4)
    return (px[:, None, None] * py[None, :, None] * pz[None, None, :]).reshape(64)


def _polish(C, sols):
    """Newton (Gauss-Newton on the ten cubics, zero residual at a solution) from an eigenvector's (x, y, z): takes out what the conditioning
    of the action matrix left in"""
    k = np.arange(1, 4)
    dC = [np.zeros_like(C), np.zeros_like(C), np.zeros_like(C)]
    dC[0][:, :3] = C[:, 1:] * k[None, :, None, None]; dC[1][:, :, :3] = C[:, :, 1:] * k[None, None, :, None]; dC[2][:, :, :, :3] = C[:, :, :, 1:] * k[None, None, None, :]
    Cf = C.reshape(10, 64); dCf = np.concatenate([d.reshape(10, 64) for d in dC])          # (30, 64)
    out = []
    for s in sols:
        s = np.array(s, float)
        for _ in range(3):
            m = _monomials(s)
            step = np.linalg.lstsq((dCf @ m).reshape(3, 10).T, -(Cf @ m), rcond=None)[0]
            if not np.isfinite(step).all(): break
            s = s + step
        out.append(s)
    return out


def solve_full(u5, v5):
    """-> (Es [list of (3,3), unit Frobenius norm, ascending z], xyz (m,3), all eigenvalues (complex), B); [] when the sample is degenerate"""
    B = nullspace(u5, v5)
    C = cubics(B)
    M = np.array([[c[m] for m in DEG3 + LOW] for c in C])
    try:
        T = np.linalg.solve(M[:, :10], M[:, 10:])          # DEG3[i] = -T[i] . LOW
    except np.linalg.LinAlgError:
        return [], np.zeros((0, 3)), np.zeros(0, complex), B
    A = np.zeros((10, 10))
    for j, m in enumerate(LOW):                            # x * LOW[j] in the basis LOW
        mx = (m[0] + 1, m[1], m[2])
        if mx in LOW: A[j, LOW.index(mx)] = 1.0
        else: A[j] = -T[DEG3.index(mx)]
    w, V = np.linalg.eig(A)
    sols = []
    for k in range(10):
        if not abs(w[k].imag) <= 1e-9 * (1.0 + abs(w[k].real)): continue
        vec = V[:, k] / V[9, k]
        sols.append(np.real(vec[6:9]))
    sols = _polish(C, sols)
    sols.sort(key=lambda s: s[2])
    Es = []
    for s in sols:
        p = B @ np.array([s[0], s[1], s[2], 1.0])
        E = p.reshape(3, 3).T
        Es.append(E / np.linalg.norm(E))
    return Es, np.array(sols).reshape(-1, 3), w, B


def solve(u5, v5):
    return solve_full(u5, v5)[0]


def sign_distance(E1, E2):
    return min(np.linalg.norm(E1 - E2), np.linalg.norm(E1 + E2))


def sample_is_unstable(Es, w):
    """a sample the solver probe test leaves out: two solutions closer than 1e-6, or an eigenvalue with |imag| between 1e-12 and 1e-6"""
    for i in range(len(Es)):
        for j in range(i):
            if sign_distance(Es[i], Es[j]) < 1e-6: return True
    im = np.abs(w.imag)
    return bool(((im > 1e-12) & (im < 1e-6)).any())


def residual(E, u, v):
    u = np.asarray(u); v = np.asarray(v)
    line = (u / u[..., 2:3]) @ E.T
    d = np.sum(v * line, axis=-1)
    return d * d / (line[..., 0] ** 2 + line[..., 1] ** 2)


def decompose(E):
    """-> R1, R2, t: the largest entry of t positive (first of equals), R1 the rotation with <[t]x R1, E> > 0"""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0: U = -U
    if np.linalg.det(Vt) < 0: Vt = -Vt
    W = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2] / np.linalg.norm(U[:, 2])
    if t[np.argmax(np.abs(t))] < 0: t = -t
    S = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    if np.sum((S @ R1) * E) < 0: R1, R2 = R2, R1
    return R1, R2, t


def cheirality(R, t, p1, p2):
    P2 = np.hstack([R, t[:, None]])
    A = np.array([[-1.0, 0, p1[0], 0], [0, -1.0, p1[1], 0], p2[0] * P2[2] - P2[0], p2[1] * P2[2] - P2[1]])
    h = np.linalg.svd(A)[2][3]
    X = h[:3] / h[3]
    lo, hi = np.finfo(float).eps, 1000.0 * np.linalg.norm(R.T @ t)
    d1 = X[2]
    if not (lo < d1 < hi): return False
    d2 = (P2[2, :3] @ X + P2[2, 3]) * np.linalg.norm(P2[:, 2])
    return bool(lo < d2 < hi)


def pose_from_E(E, u, v, inliers):
    """-> R, t, votes (4,): candidates (R1, t) (R2, t) (R1, -t) (R2, -t), the last with the largest vote wins"""
    R1, R2, t = decompose(E)
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    votes = np.zeros(4, int)
    with np.errstate(all="ignore"):
        for q in inliers:
            p1, p2 = u[q, :2] / u[q, 2], v[q, :2] / v[q, 2]
            for c, (R, tt) in enumerate(cands): votes[c] += cheirality(R, tt, p1, p2)
    best, bv = 0, 0
    for c in range(4):
        if votes[c] >= bv: bv, best = votes[c], c
    return cands[best][0], cands[best][1], votes


class Stream:
    """std::mt19937(seed) + uniform_int_distribution<int>(lo, hi) draws in sequence; oracle.mt19937_draws replays a whole list of ranges from
    the seed, so the ranges asked so far are kept and the list is extended speculatively"""
    def __init__(self, seed):
        from oracle import oracle as O
        self.O, self.seed, self.ranges, self.spec, self.vals = O, seed, [], [], []

    def _need(self, upcoming):
        k = len(self.ranges)
        if self.spec[k:k + len(upcoming)] != upcoming:
            self.spec = self.ranges + upcoming
            lo = [r[0] for r in self.spec]; hi = [r[1] for r in self.spec]
            self.vals = list(self.O.mt19937_draws(self.seed, lo, hi)[1])

    def draw(self, lo, hi, lookahead=512):
        k = len(self.ranges)
        if k >= len(self.spec) or self.spec[k] != (lo, hi): self._need([(lo, hi)] * lookahead)
        self.ranges.append((lo, hi))
        return int(self.vals[k])

    def shuffle(self, lst):
        """utils::RandomShuffle: Fisher-Yates, draw i uniform in [i, m-1]"""
        m = len(lst)
        if m < 2: return
        self._need([(i, m - 1) for i in range(m - 1)])
        for i in range(m - 1):
            j = self.draw(i, m - 1); lst[i], lst[j] = lst[j], lst[i]


def num_required_iterations(ratio, pmiss, ssize, mn, mx):
    if ratio <= 0.0: return mx
    if ratio >= 1.0: return mn
    pn = 1.0 - ratio ** ssize
    if pn >= 0.99999999999999: return mx
    it = np.ceil(np.log(pmiss) / np.log(pn) + 0.5)
    return int(max(mn, min(it, mx)))


def replay(u, v, sq_thresh, seed=0, min_num_inliers=0, min_it=100, max_it=10000, success_prob=0.9999, thresh_mult=2.0 ** 0.5, lo_start=50, rel=1e-9):
    """-> dict(E, score, mask, num_inliers, iterations, lo_runs, R, t, accepted, marginal).  marginal: some `score < best` comparison, or some
    residual against a threshold, was decided by less than the relative `rel`."""
    u = np.asarray(u, float); v = np.asarray(v, float); n = len(u)
    MAXD = np.finfo(float).max
    out = dict(E=np.zeros((3, 3)), score=MAXD, mask=np.zeros(n, bool), num_inliers=0, iterations=0, lo_runs=0, R=np.eye(3), t=np.zeros(3),
               accepted=False, marginal=False)
    if n < 5: return out
    flag = [False]

    def less(a, b):
        # (equal: every residual clipped on both sides.  Scores that differ by less than rel * threshold are rounding noise of exact fits.)
        if a < MAXD and b < MAXD and a != b and abs(a - b) <= rel * max(abs(a), abs(b), sq_thresh): flag[0] = True
        return a < b

    def res_below(E, thr):
        with np.errstate(all="ignore"): r = residual(E, u, v)
        if (np.abs(r - thr) <= rel * thr).any(): flag[0] = True
        return r < thr

    def score(E):
        with np.errstate(all="ignore"): r = residual(E, u, v)
        return float(np.sum(np.fmin(r, sq_thresh)))

    sampler, rng = Stream(seed), Stream(seed)
    draw_better = (n / (n - 5) < np.e) if n > 5 else False

    def sample():
        if draw_better:
            s = []
            while len(s) < 5:
                d = sampler.draw(0, n - 1)
                if d not in s: s.append(d)
            return s
        p = list(range(n))
        if n != 5: sampler.shuffle(p)
        return p[:5]

    def local_optimization(model):
        if 6 > n: return
        inl = list(np.nonzero(res_below(model, sq_thresh * thresh_mult))[0])      # LeastSquaresFit
        if len(inl) < 5: return
        rng.shuffle(inl)                                                          # RandomShuffleAndResize; LeastSquares is empty
        # ScoreModel(m_init) equals the model's own score: UpdateBestModel changes nothing; num_lo_steps_ = 0

    best, best_score, lo_runs = None, MAXD, 0
    max_iter, it = max(max_it, min_it), 0

    def refresh():
        ni = int(res_below(best, sq_thresh).sum())
        return num_required_iterations(ni / n, 1.0 - success_prob, 5, min_it, max_it)

    while it < max_iter:
        if it == lo_start and best_score < MAXD:
            lo_runs += 1; local_optimization(best); max_iter = refresh()
        s = sample()
        Es = solve(u[s], v[s])
        if len(Es) > 0:
            bl, bm = MAXD, 0
            for m, E in enumerate(Es):
                sc = score(E)
                if less(sc, bl): bl, bm = sc, m
            if less(bl, best_score) or it == lo_start:
                best_min = bl < best_score
                if best_min: best_score, best = bl, Es[bm]
                run_lo = it >= lo_start and best_score < MAXD
                if best_min or run_lo:
                    if run_lo: lo_runs += 1; local_optimization(best)
                    max_iter = refresh()
        it += 1
    if it <= lo_start and best_score < MAXD:
        lo_runs += 1; local_optimization(best)
    out["iterations"], out["lo_runs"] = it, lo_runs
    if best is None:
        out["marginal"] = flag[0]
        return out
    mask = res_below(best, sq_thresh)
    out.update(E=best, score=best_score, mask=mask, num_inliers=int(mask.sum()))
    if out["num_inliers"] > min_num_inliers:
        R, t, _ = pose_from_E(best, u, v, np.nonzero(mask)[0])
        out.update(R=R, t=t, accepted=True)
    out["marginal"] = flag[0]
    return out
