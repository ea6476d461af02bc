// spherical_sfm_amd -- device functions of the general (five-point) relative-pose path, shared by k_lomsac5_trace and its probes (fivepoint.hip):
//   SteweniusEstimator::MinimalSolver                     evaluation/five_point/stewenius_estimator.cpp:13-62
//   FivePointEstimator::EvaluateModelOnPoint              evaluation/five_point/five_point_estimator.cpp:115-125
//   DecomposeEssentialMatrix / PoseFromEssentialMatrix    evaluation/five_point/five_point_estimator.cpp:15-113
// The reference's solver is 600 lines of generated coefficient code over Eigen; none of it is restated.  The solver here is derived from
// the mathematics ("General relative pose"): nullspace -> the ten cubic constraints by polynomial arithmetic -> Gauss-Jordan on the 10 x 20
// coefficient matrix -> a 3 x 3 polynomial matrix in z -> its degree-10 determinant -> real roots bracketed between the roots of the
// derivatives -> (x, y) from the nullvector of the 3 x 3 matrix at each root.  REAL solutions only (ssfm.h says what that changes).
// 3x3 matrices are row-major here.
#pragma once
#ifndef FP_HOST_HARNESS          // tests/native/fivepoint_host.cpp compiles this header for the CPU and brings the few helpers it needs itself
#include "ransac_device.h"
#endif
#ifndef FP_POLISH_STEPS
#define FP_POLISH_STEPS 4        // Gauss-Newton steps of fp_polish (0 in the host harness shows what the elimination alone delivers)
#endif

namespace ssfm {

constexpr double FP_RANK_TOL = 1e-10;     // a unit-length row of the 5x9 system whose part outside the span of the rows before it is shorter: rank-deficient, 0 models
constexpr double FP_PIVOT_TOL = 1e-12;    // Gauss-Jordan pivot of the 10x20 system (built from an orthonormal basis: entries O(1)) below it: 0 models
constexpr double FP_ROOT_BOUND = 1e12;    // real roots of the degree-10 polynomial are searched in [-1e12, 1e12]

// ---- polynomials in (x, y, z, 1) as homogeneous forms in four variables 0 = x, 1 = y, 2 = z, 3 = 1 -------------------------------
// linear: 4 coefficients; quadratic: 10, entry (a <= b); cubic: column of the 10x20 system from the exponents.
__host__ __device__ constexpr int fp_qidx(int a, int b) { return (a == 0 ? 0 : a == 1 ? 4 : a == 2 ? 7 : 9) + (b - a); }
// columns: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1  (the first ten are eliminated; what is left
// of rows 4..9 is linear in x and y with polynomial coefficients in z)
__host__ __device__ constexpr int fp_ccol(int ex, int ey, int ez) {
    switch (ex * 16 + ey * 4 + ez) {
        case 48: return 0;  case 12: return 1;  case 36: return 2;  case 24: return 3;  case 33: return 4;
        case 32: return 5;  case 9: return 6;   case 8: return 7;   case 21: return 8;  case 20: return 9;
        case 18: return 10; case 17: return 11; case 16: return 12; case 6: return 13;  case 5: return 14;
        case 4: return 15;  case 3: return 16;  case 2: return 17;  case 1: return 18;  default: return 19;
    }
}
__host__ __device__ constexpr int fp_ccol3(int a, int b, int c) {
    return fp_ccol((a == 0) + (b == 0) + (c == 0), (a == 1) + (b == 1) + (c == 1), (a == 2) + (b == 2) + (c == 2));
}
// q += s * l1 * l2
__device__ __forceinline__ void fp_quad_acc(double* q, const double* l1, const double* l2, double s) {
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) q[fp_qidx(a < b ? a : b, a < b ? b : a)] += s * l1[a] * l2[b];
}
// row (20 columns) += s * q * l
__device__ __forceinline__ void fp_cubic_acc(double* row, const double* q, const double* l, double s) {
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = a; b < 4; b++)
#pragma unroll
            for (int c = 0; c < 4; c++) row[fp_ccol3(a, b, c)] += s * q[fp_qidx(a, b)] * l[c];
}

// Orthonormal basis B (9x4, B[k][a]) of the right nullspace of the 5x9 matrix with rows [u0v0 u0v1 u0v2 u1v0 ... u2v2].  The five rows are
// orthonormalised (Gram-Schmidt, every projection twice), then four unit vectors e_k -- each time the one with the largest part outside
// everything found so far -- are orthonormalised against all of it.  false: rank-deficient.
__device__ bool fp_nullspace(const double* u5, const double* v5, double (*B)[4]) {
    double Q[9][9];
    for (int i = 0; i < 5; i++) {
        double nn = 0.0;
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) { const double x = u5[3 * i + a] * v5[3 * i + b]; Q[i][3 * a + b] = x; nn += x * x; }
        if (!(nn > 0.0) || !isfinite(nn)) return false;
        const double s = 1.0 / sqrt(nn);
        for (int k = 0; k < 9; k++) Q[i][k] *= s;
        for (int pass = 0; pass < 2; pass++)
            for (int j = 0; j < i; j++) { double d = 0.0; for (int k = 0; k < 9; k++) d += Q[i][k] * Q[j][k]; for (int k = 0; k < 9; k++) Q[i][k] -= d * Q[j][k]; }
        double rn = 0.0; for (int k = 0; k < 9; k++) rn += Q[i][k] * Q[i][k];
        if (!(rn > FP_RANK_TOL * FP_RANK_TOL)) return false;
        const double r = 1.0 / sqrt(rn);
        for (int k = 0; k < 9; k++) Q[i][k] *= r;
    }
    for (int t = 0; t < 4; t++) {
        const int i = 5 + t;
        int best = 0; double bres = -1.0;
        for (int k = 0; k < 9; k++) { double s = 1.0; for (int j = 0; j < i; j++) s -= Q[j][k] * Q[j][k]; if (s > bres) { bres = s; best = k; } }
        for (int k = 0; k < 9; k++) Q[i][k] = (k == best) ? 1.0 : 0.0;
        for (int pass = 0; pass < 2; pass++)
            for (int j = 0; j < i; j++) { double d = 0.0; for (int k = 0; k < 9; k++) d += Q[i][k] * Q[j][k]; for (int k = 0; k < 9; k++) Q[i][k] -= d * Q[j][k]; }
        double rn = 0.0; for (int k = 0; k < 9; k++) rn += Q[i][k] * Q[i][k];
        const double r = 1.0 / sqrt(rn);                    // rn >= (4 - t) / 9 up to rounding
        for (int k = 0; k < 9; k++) { Q[i][k] *= r; B[k][t] = Q[i][k]; }
    }
    return true;
}

// polynomial in z, ascending coefficients: value and derivative
__device__ __forceinline__ double fp_horner(const double* c, int deg, double z) { double p = c[deg]; for (int k = deg - 1; k >= 0; k--) p = fma(p, z, c[k]); return p; }
__device__ __forceinline__ void fp_horner2(const double* c, int deg, double z, double* p, double* dp) {
    double a = c[deg], b = 0.0;
    for (int k = deg - 1; k >= 0; k--) { b = fma(b, z, a); a = fma(a, z, c[k]); }
    *p = a; *dp = b;
}
// Real roots of c (degree 10, ascending coefficients) in ascending order.  The roots of the (10 - d)-th derivative separate those of the
// (9 - d)-th, so the derivatives are solved from the linear one up; inside a bracket with a sign change: Newton, bisection when Newton leaves it.
// A root of even multiplicity has no sign change and is not found: it is a solution about to become complex.
__device__ int fp_real_roots10(const double* c, double* roots) {
    double prev[10], cur[10], q[11];
    int nprev = 0;
    for (int d = 1; d <= 10; d++) {
        const int m = 10 - d;                                  // q = m-th derivative of c, degree d
        for (int j = 0; j <= d; j++) { double f = c[j + m]; for (int k = 0; k < m; k++) f *= (double)(j + m - k); q[j] = f; }
        int ncur = 0;
        if (q[d] != 0.0 && isfinite(q[d])) {
            double bound = 0.0; for (int j = 0; j < d; j++) bound = fmax(bound, fabs(q[j] / q[d]));
            bound = fmin(1.0 + bound, FP_ROOT_BOUND);
            if (!(bound >= 1.0)) bound = FP_ROOT_BOUND;        // NaN
            double a = -bound, fa = fp_horner(q, d, a);
            for (int s = 0; s <= nprev; s++) {
                double b = (s < nprev) ? prev[s] : bound;
                if (b > bound) b = bound;
                if (!(b > a)) continue;
                const double fb = fp_horner(q, d, b);
                if (fa != 0.0 && fb != 0.0 && ((fa < 0.0) != (fb < 0.0))) {
                    // safeguarded Newton: a bisection step whenever Newton would leave the bracket or does not halve the step
                    double lo = a, hi = b; const bool up = fa < 0.0;       // q(lo) and q(hi) keep their signs
                    double x = 0.5 * (lo + hi), dxold = hi - lo, dx = dxold, p, dp;
                    fp_horner2(q, d, x, &p, &dp);
                    for (int it = 0; it < 300 && p != 0.0; it++) {
                        if ((p < 0.0) == up) lo = x; else hi = x;
                        const bool bisect = (((x - hi) * dp - p) * ((x - lo) * dp - p) > 0.0) || (fabs(2.0 * p) > fabs(dxold * dp)) || !isfinite(dp);
                        dxold = dx;
                        if (bisect) { dx = 0.5 * (hi - lo); x = lo + dx; } else { dx = p / dp; x -= dx; }
                        if (fabs(dx) <= 2.3e-16 * fabs(x) + 1e-300) break;
                        fp_horner2(q, d, x, &p, &dp);
                    }
                    cur[ncur++] = x;
                }
                a = b; fa = fb;
            }
        } else {                                               // the leading coefficient vanished: the critical points carry over
            for (int s = 0; s < nprev; s++) cur[ncur++] = prev[s];
        }
        nprev = ncur; for (int s = 0; s < ncur; s++) prev[s] = cur[s];
    }
    for (int s = 0; s < nprev; s++) roots[s] = prev[s];
    return nprev;
}

// Gauss-Newton on the ten constraints themselves at a root (x, y, z) of the eliminated system: f(E) = [det E; 2 E E^T E - tr(E E^T) E] with
// E = x E1 + y E2 + z E3 + E4, three unknowns, zero residual at a solution -- so the steps converge quadratically and the solution no
// longer carries the conditioning of the degree-10 polynomial it was found with.  At most four steps.
__device__ void fp_polish(const double (*B)[4], double* xyz) {
    for (int it = 0; it < FP_POLISH_STEPS; it++) {
        double E[9], D[3][9];
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) {
            const double* b = B[r + 3 * c];
            E[3 * r + c] = b[0] * xyz[0] + b[1] * xyz[1] + b[2] * xyz[2] + b[3];
            D[0][3 * r + c] = b[0]; D[1][3 * r + c] = b[1]; D[2][3 * r + c] = b[2];
        }
        double G[9], f[10], J[10][3], cof[9];
        mat3_mul_bt(E, E, G);
        const double tr = G[0] + G[4] + G[8];
        cof[0] = E[4] * E[8] - E[5] * E[7]; cof[1] = E[5] * E[6] - E[3] * E[8]; cof[2] = E[3] * E[7] - E[4] * E[6];
        cof[3] = E[2] * E[7] - E[1] * E[8]; cof[4] = E[0] * E[8] - E[2] * E[6]; cof[5] = E[1] * E[6] - E[0] * E[7];
        cof[6] = E[1] * E[5] - E[2] * E[4]; cof[7] = E[2] * E[3] - E[0] * E[5]; cof[8] = E[0] * E[4] - E[1] * E[3];
        f[0] = E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2];
        double GE[9]; mat3_mul(G, E, GE);
        for (int k = 0; k < 9; k++) f[1 + k] = 2.0 * GE[k] - tr * E[k];
        for (int a = 0; a < 3; a++) {
            double dG[9], t1[9], t2[9], t3[9];
            mat3_mul_bt(D[a], E, t1); mat3_mul_bt(E, D[a], t2);
            for (int k = 0; k < 9; k++) dG[k] = t1[k] + t2[k];
            const double dtr = dG[0] + dG[4] + dG[8];
            mat3_mul(dG, E, t1); mat3_mul(G, D[a], t3);
            double j0 = 0.0; for (int k = 0; k < 9; k++) j0 += cof[k] * D[a][k];
            J[0][a] = j0;
            for (int k = 0; k < 9; k++) J[1 + k][a] = 2.0 * (t1[k] + t3[k]) - dtr * E[k] - tr * D[a][k];
        }
        double N[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
        for (int k = 0; k < 10; k++) for (int a = 0; a < 3; a++) { g[a] += J[k][a] * f[k]; for (int b = 0; b < 3; b++) N[3 * a + b] += J[k][a] * J[k][b]; }
        const double dN = det3_dev(N);
        if (!(fabs(dN) > 0.0) || !isfinite(dN)) return;
        double c0[3], c1[3], c2[3];
        cross3(N + 3, N + 6, c0); cross3(N + 6, N, c1); cross3(N, N + 3, c2);            // rows of adj(N)^T; N is symmetric
        const double dx = -(c0[0] * g[0] + c0[1] * g[1] + c0[2] * g[2]) / dN, dy = -(c1[0] * g[0] + c1[1] * g[1] + c1[2] * g[2]) / dN,
                     dz = -(c2[0] * g[0] + c2[1] * g[1] + c2[2] * g[2]) / dN;
        if (!isfinite(dx) || !isfinite(dy) || !isfinite(dz)) return;
        xyz[0] += dx; xyz[1] += dy; xyz[2] += dz;
        if (fabs(dx) + fabs(dy) + fabs(dz) <= 1e-15 * (1.0 + fabs(xyz[0]) + fabs(xyz[1]) + fabs(xyz[2]))) return;
    }
}

// SteweniusEstimator::MinimalSolver on five rays (u5, v5: 5 x 3): the real essential matrices with v^T E u = 0, each of unit Frobenius
// norm, at most ten, in ascending order of z where E = x E1 + y E2 + z E3 + E4 over the nullspace basis.  Es: [count][9] row-major.
__device__ int fp_minimal_solver(const double* u5, const double* v5, double* Es) {
    double B[9][4];
    if (!fp_nullspace(u5, v5, B)) return 0;
    // E(r, c) = p[r + 3c]  (stewenius_estimator.cpp:47-51), p = B (x, y, z, 1)^T
    double M[10][20];
    for (int r = 0; r < 10; r++) for (int k = 0; k < 20; k++) M[r][k] = 0.0;
#define FP_E(r, c) (&B[(r) + 3 * (c)][0])
    {   // det E = 0
        double q[10];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int j = (i + 1) % 3, k = (i + 2) % 3;           // row 0 expansion: E0i (E1j E2k - E1k E2j), cyclic
            for (int t = 0; t < 10; t++) q[t] = 0.0;
            fp_quad_acc(q, FP_E(1, j), FP_E(2, k), 1.0); fp_quad_acc(q, FP_E(1, k), FP_E(2, j), -1.0);
            fp_cubic_acc(M[0], q, FP_E(0, i), 1.0);
        }
    }
    {   // 2 E E^T E - tr(E E^T) E = 0: L = 2 E E^T - tr(E E^T) I (quadratics), rows 1..9 = (L E)(i, j)
        double L[3][3][10];
        for (int i = 0; i < 3; i++) for (int j = i; j < 3; j++) {
            for (int t = 0; t < 10; t++) L[i][j][t] = 0.0;
            for (int k = 0; k < 3; k++) fp_quad_acc(L[i][j], FP_E(i, k), FP_E(j, k), 1.0);
        }
        for (int t = 0; t < 10; t++) {
            const double tr = L[0][0][t] + L[1][1][t] + L[2][2][t];
            for (int i = 0; i < 3; i++) for (int j = i; j < 3; j++) L[i][j][t] = 2.0 * L[i][j][t] - (i == j ? tr : 0.0);
            L[1][0][t] = L[0][1][t]; L[2][0][t] = L[0][2][t]; L[2][1][t] = L[1][2][t];
        }
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) fp_cubic_acc(M[1 + 3 * i + j], L[i][k], FP_E(k, j), 1.0);
    }
#undef FP_E
    // Gauss-Jordan on the first ten columns, partial pivoting over the rows
    for (int k = 0; k < 10; k++) {
        int pr = k; double pv = fabs(M[k][k]);
        for (int r = k + 1; r < 10; r++) { const double a = fabs(M[r][k]); if (a > pv) { pv = a; pr = r; } }
        if (!(pv >= FP_PIVOT_TOL)) return 0;
        if (pr != k) for (int j = k; j < 20; j++) { const double t = M[k][j]; M[k][j] = M[pr][j]; M[pr][j] = t; }
        const double inv = 1.0 / M[k][k];
        for (int j = k; j < 20; j++) M[k][j] *= inv;
        for (int r = 0; r < 10; r++) {
            if (r == k) continue;
            const double f = M[r][k];
            if (f != 0.0) for (int j = k; j < 20; j++) M[r][j] -= f * M[k][j];
        }
    }
    // rows (4, 5), (6, 7), (8, 9): [x^2 z | x^2], [y^2 z | y^2], [xyz | xy]; (first) - z (second) = x px(z) + y py(z) + p1(z)
    double P[3][3][5];                                         // [row][x | y | 1][power of z]
    for (int i = 0; i < 3; i++) {
        const double* a = &M[4 + 2 * i][10]; const double* b = &M[5 + 2 * i][10];
        for (int g = 0; g < 2; g++) {                          // tail columns of x: z^2 z 1, of y likewise
            P[i][g][0] = a[3 * g + 2]; P[i][g][1] = a[3 * g + 1] - b[3 * g + 2]; P[i][g][2] = a[3 * g] - b[3 * g + 1]; P[i][g][3] = -b[3 * g]; P[i][g][4] = 0.0;
        }
        P[i][2][0] = a[9]; P[i][2][1] = a[8] - b[9]; P[i][2][2] = a[7] - b[8]; P[i][2][3] = a[6] - b[7]; P[i][2][4] = -b[6];
    }
    double det[11]; for (int k = 0; k < 11; k++) det[k] = 0.0;
    for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        double cof[7]; for (int t = 0; t < 7; t++) cof[t] = 0.0;
        for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) cof[a + b] += P[j][0][a] * P[k][1][b] - P[j][1][a] * P[k][0][b];
        for (int a = 0; a < 5; a++) for (int b = 0; b < 7; b++) det[a + b] += P[i][2][a] * cof[b];
    }
    double roots[10];
    const int nr = fp_real_roots10(det, roots);
    int cnt = 0;
    for (int s = 0; s < nr; s++) {
        const double z = roots[s];
        double rw[3][3];
        for (int i = 0; i < 3; i++) { rw[i][0] = fp_horner(P[i][0], 3, z); rw[i][1] = fp_horner(P[i][1], 3, z); rw[i][2] = fp_horner(P[i][2], 4, z); }
        double bx = 0.0, by = 0.0, bw = 0.0;
        for (int i = 0; i < 3; i++) {
            const int j = (i + 1) % 3; double cr[3]; cross3(rw[i], rw[j], cr);
            if (fabs(cr[2]) > fabs(bw)) { bx = cr[0]; by = cr[1]; bw = cr[2]; }
        }
        if (bw == 0.0) continue;
        double xyz[3] = {bx / bw, by / bw, z};
        fp_polish(B, xyz);
        double p[9], nn = 0.0;
        for (int k = 0; k < 9; k++) { p[k] = B[k][0] * xyz[0] + B[k][1] * xyz[1] + B[k][2] * xyz[2] + B[k][3]; nn += p[k] * p[k]; }
        if (!(nn > 0.0) || !isfinite(nn)) continue;
        const double sc = 1.0 / sqrt(nn);
        double* E = Es + 9 * cnt;
        for (int r = 0; r < 3; r++) for (int cidx = 0; cidx < 3; cidx++) E[3 * r + cidx] = p[r + 3 * cidx] * sc;
        cnt++;
    }
    return cnt;
}

// FivePointEstimator::EvaluateModelOnPoint (five_point_estimator.cpp:115-125) with a = u0 / u2, b = u1 / u2 already divided (u2 / u2 = 1):
// line = E (a, b, 1), d = v . line, d^2 / (line0^2 + line1^2).  One-sided; v is not renormalised.  The operation order is spelled out with
// fma so that every caller -- rays in LDS or in global memory, probe or trace -- gets the same bits.
__device__ __forceinline__ double fp_residual_n(const double* E, double a, double b, double v0, double v1, double v2) {
    const double l0 = fma(E[0], a, fma(E[1], b, E[2])), l1 = fma(E[3], a, fma(E[4], b, E[5])), l2 = fma(E[6], a, fma(E[7], b, E[8]));
    const double d = fma(v0, l0, fma(v1, l1, v2 * l2));
    return (d * d) / fma(l0, l0, l1 * l1);
}
__device__ __forceinline__ double fp_residual(const double* E, const double* u, const double* v) { return fp_residual_n(E, u[0] / u[2], u[1] / u[2], v[0], v[1], v[2]); }

// where the rays of a pair are: raw u and v in global memory (RAYS_LDS = false), or (u0/u2, u1/u2) and v staged in LDS (5 doubles per ray)
template <bool RAYS_LDS>
struct FpRays {
    const double* gu; const double* gv; const double* sn; const double* sv;
    __device__ __forceinline__ void get(int i, double* a, double* b, double* v0, double* v1, double* v2) const {
        if (RAYS_LDS) { *a = sn[2 * i]; *b = sn[2 * i + 1]; *v0 = sv[3 * i]; *v1 = sv[3 * i + 1]; *v2 = sv[3 * i + 2]; }
        else { const double u2 = gu[3 * i + 2]; *a = gu[3 * i] / u2; *b = gu[3 * i + 1] / u2; *v0 = gv[3 * i]; *v1 = gv[3 * i + 1]; *v2 = gv[3 * i + 2]; }
    }
    __device__ __forceinline__ double residual(const double* E, int i) const { double a, b, v0, v1, v2; get(i, &a, &b, &v0, &v1, &v2); return fp_residual_n(E, a, b, v0, v1, v2); }
};

// One-sided Jacobi SVD of an N x N matrix, the iteration retriangulate.hip runs for its DLT (pairs (p, q) in row order per sweep, until the
// largest normalised column product of a sweep is below 1e-15, at most 60 sweeps): A <- A V with orthogonal columns, V accumulated.
template <int N>
__device__ void fp_jacobi(double (*A)[N], double (*V)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int i = 0; i < N; i++) { alpha += A[i][p] * A[i][p]; beta += A[i][q] * A[i][q]; gamma += A[i][p] * A[i][q]; }
                if (gamma != 0.0) {
                    const double rel = fabs(gamma) / sqrt(alpha * beta + 1e-300);
                    off = (off < rel) ? rel : off;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta)), cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                    for (int i = 0; i < N; i++) { const double ap = A[i][p], aq = A[i][q]; A[i][p] = cs * ap - sn * aq; A[i][q] = sn * ap + cs * aq; }
#pragma unroll
                    for (int i = 0; i < N; i++) { const double vp = V[i][p], vq = V[i][q]; V[i][p] = cs * vp - sn * vq; V[i][q] = sn * vp + cs * vq; }
                }
            }
        if (off < 1e-15) break;
    }
}

// DecomposeEssentialMatrix (five_point_estimator.cpp:15-34): E = U diag(s, s, 0) V^T, R1 = U W V^T, R2 = U W^T V^T, t = U.col(2), both
// factors made proper.  With two equal singular values the SVD -- and with it which rotation is called R1 and the sign of t -- is the SVD
// routine's choice, so the outcome is put into a form that does not depend on it: the entry of t of largest magnitude is positive (the
// first of equals), and R1 is the rotation with <[t]x R1, E> > 0.  {R1, R2} and +-t as sets are the reference's.
__device__ void fp_decompose(const double* E, double* R1, double* R2, double* t) {
    double A[3][3], V[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) A[i][j] = E[3 * i + j];
    fp_jacobi<3>(A, V);
    double nn[3]; for (int q = 0; q < 3; q++) nn[q] = A[0][q] * A[0][q] + A[1][q] * A[1][q] + A[2][q] * A[2][q];
    int o0 = 0; for (int q = 1; q < 3; q++) if (nn[q] > nn[o0]) o0 = q;
    int o2 = (o0 == 0) ? 1 : 0; for (int q = 0; q < 3; q++) if (q != o0 && nn[q] < nn[o2]) o2 = q;
    const int o1 = 3 - o0 - o2;
    double U[9], Vt[9], u0[3], u1[3], u2[3];
    const double s0 = 1.0 / sqrt(nn[o0]), s1 = 1.0 / sqrt(nn[o1]);
    for (int i = 0; i < 3; i++) { u0[i] = A[i][o0] * s0; u1[i] = A[i][o1] * s1; }
    cross3(u0, u1, u2);                                        // the third singular value is zero: the column is completed, det U = +1
    { const double n2 = 1.0 / norm3(u2); for (int i = 0; i < 3; i++) u2[i] *= n2; }
    for (int i = 0; i < 3; i++) { U[3 * i] = u0[i]; U[3 * i + 1] = u1[i]; U[3 * i + 2] = u2[i]; Vt[i] = V[i][o0]; Vt[3 + i] = V[i][o1]; Vt[6 + i] = V[i][o2]; }
    if (det3_dev(Vt) < 0) for (int i = 0; i < 9; i++) Vt[i] = -Vt[i];
    const double W[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1}, WT[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    double UW[9];
    mat3_mul(U, W, UW); mat3_mul(UW, Vt, R1); mat3_mul(U, WT, UW); mat3_mul(UW, Vt, R2);
    t[0] = u2[0]; t[1] = u2[1]; t[2] = u2[2];
    int big = 0; for (int k = 1; k < 3; k++) if (fabs(t[k]) > fabs(t[big])) big = k;
    if (t[big] < 0) for (int k = 0; k < 3; k++) t[k] = -t[k];
    // <[t]x R1, E>
    double s = 0.0;
    for (int j = 0; j < 3; j++) {
        const double c[3] = {R1[j], R1[3 + j], R1[6 + j]}; double tc[3]; cross3(t, c, tc);
        s += tc[0] * E[j] + tc[1] * E[3 + j] + tc[2] * E[6 + j];
    }
    if (s < 0) for (int i = 0; i < 9; i++) { const double x = R1[i]; R1[i] = R2[i]; R2[i] = x; }
}

// CheckCheirality's test of one correspondence (five_point_estimator.cpp:51-86): DLT triangulation against [I | 0] and [R | t] (the last
// right singular vector of the 4x4 system, hnormalized), both depths in (epsilon, 1000 |R^T t|).  p1 = u.head(2) / u2, p2 = v.head(2) / v2.
__device__ bool fp_cheirality(const double* R, const double* t, double p1x, double p1y, double p2x, double p2y) {
    double A[4][4], V[4][4];
    A[0][0] = -1.0; A[0][1] = 0.0; A[0][2] = p1x; A[0][3] = 0.0;
    A[1][0] = 0.0; A[1][1] = -1.0; A[1][2] = p1y; A[1][3] = 0.0;
    for (int k = 0; k < 3; k++) { A[2][k] = p2x * R[6 + k] - R[k]; A[3][k] = p2y * R[6 + k] - R[3 + k]; }
    A[2][3] = p2x * t[2] - t[0]; A[3][3] = p2y * t[2] - t[1];
    fp_jacobi<4>(A, V);
    int best = 0; double bn = 1e300;
    for (int q = 0; q < 4; q++) { const double nq = A[0][q] * A[0][q] + A[1][q] * A[1][q] + A[2][q] * A[2][q] + A[3][q] * A[3][q]; if (nq < bn) { bn = nq; best = q; } }
    const double X[3] = {V[0][best] / V[3][best], V[1][best] / V[3][best], V[2][best] / V[3][best]};
    double Rtt[3]; mat3_tvec(R, t, Rtt);
    const double max_depth = 1000.0 * norm3(Rtt), min_depth = DBL_EPSILON;
    const double d1 = X[2];
    if (!(d1 > min_depth && d1 < max_depth)) return false;
    const double d2 = (R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]) * sqrt(R[2] * R[2] + R[5] * R[5] + R[8] * R[8]);
    return d2 > min_depth && d2 < max_depth;
}

// PoseFromEssentialMatrix (five_point_estimator.cpp:88-113), workgroup-cooperative: every inlier is triangulated against the four
// combinations (R1, t) (R2, t) (R1, -t) (R2, -t), the votes are integer counts in LDS, and the last combination with the largest count
// wins (the reference's >=).  The inliers are list[0 .. cnt) when list != nullptr, otherwise the i < cnt with flags[i] != 0.
// s_votes: LDS int[4].  Every thread returns the same R, t and votes.
template <bool RAYS_LDS>
__device__ void fp_pose_block(const double* E, const FpRays<RAYS_LDS>& rays, int cnt, const int* list, const unsigned char* flags, int* s_votes,
                              double* R, double* t, int* votes) {
    double R1[9], R2[9], t0[3];
    fp_decompose(E, R1, R2, t0);
    const double tn[3] = {-t0[0], -t0[1], -t0[2]};
    if (threadIdx.x < 4) s_votes[threadIdx.x] = 0;
    __syncthreads();
    int mine[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        int q = i;
        if (list) q = list[i]; else if (!flags[i]) continue;
        double a, b, v0, v1, v2; rays.get(q, &a, &b, &v0, &v1, &v2);
        const double p2x = v0 / v2, p2y = v1 / v2;
        mine[0] += fp_cheirality(R1, t0, a, b, p2x, p2y) ? 1 : 0;
        mine[1] += fp_cheirality(R2, t0, a, b, p2x, p2y) ? 1 : 0;
        mine[2] += fp_cheirality(R1, tn, a, b, p2x, p2y) ? 1 : 0;
        mine[3] += fp_cheirality(R2, tn, a, b, p2x, p2y) ? 1 : 0;
    }
    for (int c = 0; c < 4; c++) if (mine[c]) atomicAdd(&s_votes[c], mine[c]);
    __syncthreads();
    int bestc = 0, bestv = 0;
    for (int c = 0; c < 4; c++) { votes[c] = s_votes[c]; if (votes[c] >= bestv) { bestv = votes[c]; bestc = c; } }
    __syncthreads();
    const double* Rc = (bestc & 1) ? R2 : R1;
    for (int k = 0; k < 9; k++) R[k] = Rc[k];
    for (int k = 0; k < 3; k++) t[k] = (bestc & 2) ? tn[k] : t0[k];
}

}  // namespace ssfm
