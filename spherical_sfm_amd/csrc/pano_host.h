// spherical_sfm_amd -- the host plan of the stereo panorama (include/ssfm.h, "stereo panorama"): the column jobs of make_stereo_panoramas
// (examples/stereo_panorama_tools.cpp:496-616) and who owns each output column.  Plain C++, no HIP: pano.hip, the shim and tests/native/pano_host_check.cpp include it.
//
// A job is one (pair, thetanum, phinum) that passes the three angle tests of :582-592.  It is `ok` when get_synthetic_column_maps (:69-106) would return true:
// XL(2) > 0 and XR(2) > 0 on every row.  The reference writes columns pair by pair with copyTo, so the owner of output column (phinum, colout) is the ok job of the
// highest pair index; colout = (thetanum + shift(phinum)) mod pano_width is injective in thetanum, so a pair has at most one job per output column.
//
// Every transcendental (tan, sin, cos, atan2) is taken here.  What the kernel consumes per job is tan(phi) and synth_R (row-major), and from them it forms the row
// map with + - * / only, in the order written once in pano_row_map below, which the plan uses itself for `ok`.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

namespace ssfm {

struct PanoParams {
    int32_t num_phi = 9; double phi_step_deg = 1.0, depth = 10.0, synth_radius = 0.5, synth_focal_factor = 1.2; int32_t is_loop = 1;
};

struct PanoJob {
    int32_t pair, theta, phi, col; uint8_t ok; double alpha, tan_phi, synth_R[9];
};

struct PanoPlan {
    std::vector<PanoJob> jobs;          // pair-major, then thetanum, then phinum: the order in which the reference meets them
    std::vector<int32_t> owner;         // [num_phi * pano_width] pair index of the owning job, -1 = none
    std::vector<int32_t> owner_job;     // the same as an index into jobs
    int num_pairs = 0;
};

// The y-independent part of the row map of one job: world_i(y) = (p0[i] + r1[i] * d1(y)) + p2[i], d1(y) = ((y - cy) / synth_focal) * depth.
// p0[i] = synth_R[0][i] * (tan_phi * depth) and p2[i] = synth_R[2][i] * (1 * depth + synth_radius) are single products, so forming them once is the same bits as
// forming them on every row.
struct PanoRowConsts { double p0[3], r1[3], p2[3]; };

#if defined(__HIPCC__)
#define PANO_HD __host__ __device__ __forceinline__
#else
#define PANO_HD inline
#endif

PANO_HD PanoRowConsts pano_row_consts(double tan_phi, const double* synth_R, double depth, double synth_radius) {
    PanoRowConsts c;
    const double d0 = tan_phi * depth, d2 = 1.0 * depth + synth_radius;            // synth_X - synth_t, synth_t = (0, 0, -synth_radius)
    for (int i = 0; i < 3; i++) { c.p0[i] = synth_R[0 * 3 + i] * d0; c.r1[i] = synth_R[1 * 3 + i]; c.p2[i] = synth_R[2 * 3 + i] * d2; }
    return c;
}

// THE operation order of the row map (:83-99), host and device, plan and kernel:
//   sy = (y - cy) / synth_focal;  d1 = sy * depth;  world_i = (p0_i + r1_i * d1) + p2_i              (world_X = synth_R^T (synth_X - synth_t))
//   X_i = ((R_i0 * world_0 + R_i1 * world_1) + R_i2 * world_2) + t_i                                  (R row-major)
//   x = (focal * X_0) / X_2 + cx,  y = (focal * X_1) / X_2 + cy
// Compiled without contraction wherever last bits are compared (csrc/Makefile).
PANO_HD void pano_world(const PanoRowConsts& c, double y, double cy, double synth_focal, double depth, double* w) {
    const double sy = (y - cy) / synth_focal, d1 = sy * depth;
    for (int i = 0; i < 3; i++) w[i] = (c.p0[i] + c.r1[i] * d1) + c.p2[i];
}
PANO_HD void pano_camera(const double* R, const double* t, const double* w, double* X) {
    for (int i = 0; i < 3; i++) X[i] = ((R[i * 3 + 0] * w[0] + R[i * 3 + 1] * w[1]) + R[i * 3 + 2] * w[2]) + t[i];
}

namespace pano_detail {

inline void so3exp_y(double theta, double* R) {                      // so3exp((0, -theta, 0)), src/so3.cpp:16-23, row-major
    const double r[3] = {0.0, -theta, 0.0};
    const double norm = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (norm < 1e-10) return;
    const double v[3] = {r[0] / norm, r[1] / norm, r[2] / norm};
    const double K[9] = {0, -v[2], v[1], v[2], 0, -v[0], -v[1], v[0], 0};
    const double s = std::sin(norm), c1 = 1.0 - std::cos(norm);
    double cK[9], KK[9];
    for (int i = 0; i < 9; i++) cK[i] = c1 * K[i];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) KK[i * 3 + j] = cK[i * 3 + 0] * K[0 * 3 + j] + cK[i * 3 + 1] * K[1 * 3 + j] + cK[i * 3 + 2] * K[2 * 3 + j];
    for (int i = 0; i < 9; i++) R[i] = (R[i] + s * K[i]) + KK[i];
}
inline void mul_Rt(const double* R, const double* x, double* out) {  // R^T x
    for (int i = 0; i < 3; i++) out[i] = R[0 * 3 + i] * x[0] + R[1 * 3 + i] * x[1] + R[2 * 3 + i] * x[2];
}
inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline void project(const double* v, const double* up, double* out) { const double d = dot3(v, up); for (int i = 0; i < 3; i++) out[i] = v[i] - up[i] * d; }
inline void cross(const double* a, const double* b, double* c) { c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0]; }
inline double signed_angle_between(const double* a, const double* b, const double* up) { double c[3]; cross(a, b, c); return std::atan2(dot3(c, up), dot3(a, b)); }
inline void center(const double* R, const double* t, double* c) { double m[3]; mul_Rt(R, t, m); for (int i = 0; i < 3; i++) c[i] = -m[i]; }

// XL(2) > 0 and XR(2) > 0 on every row.  In exact arithmetic X(2) is affine in y, and the computed value is within 32 ulp-units of the sum B(y) of the absolute
// values of its terms; B is convex in y, so it is largest at an end.  Both ends above 1e-10 * B (4e5 times that error) therefore decide every row between them; an
// end at or below zero decides the other way, being a row itself.  Only what is left (an end in (0, 1e-10 * B]) walks all rows.
inline bool depth_positive_on_every_row(const PanoRowConsts& c, const double* R, const double* t, double cy, double synth_focal, double depth, int height) {
    double zmin = 0.0, bmax = 0.0;
    for (int e = 0; e < 2; e++) {
        const double y = e == 0 ? 0.0 : (double)(height - 1);
        double w[3], X[3]; pano_world(c, y, cy, synth_focal, depth, w); pano_camera(R, t, w, X);
        const double d1 = std::fabs(((y - cy) / synth_focal) * depth);
        double b = std::fabs(t[2]);
        for (int i = 0; i < 3; i++) b += std::fabs(R[6 + i]) * (std::fabs(c.p0[i]) + std::fabs(c.r1[i]) * d1 + std::fabs(c.p2[i]));
        if (!(X[2] > 0.0)) return false;
        zmin = e == 0 ? X[2] : std::min(zmin, X[2]); bmax = std::max(bmax, b);
    }
    if (zmin > 1e-10 * bmax) return true;
    for (int y = 1; y < height - 1; y++) {
        double w[3], X[3]; pano_world(c, (double)y, cy, synth_focal, depth, w); pano_camera(R, t, w, X);
        if (!(X[2] > 0.0)) return false;
    }
    return true;
}

}  // namespace pano_detail

inline int pano_num_pairs(int n, int is_loop) { return n <= 0 ? 0 : (is_loop ? n : n - 1); }

inline double pano_phi(const PanoParams& P, int i) {                // :485-494, with the step as a factor (step 1.0 multiplies exactly)
    if (P.num_phi == 1) return 0.0;
    const double min_phi = (-(P.num_phi - 1) / 2.) * P.phi_step_deg * M_PI / 180., max_phi = ((P.num_phi - 1) / 2.) * P.phi_step_deg * M_PI / 180.;
    return min_phi + i * (max_phi - min_phi) / (P.num_phi - 1);
}

// What the reference recomputes for every pair but depends on thetanum (and phinum) alone: synth_R, the synthetic centre, the projected synthetic rays.
struct PanoThetaTable {
    std::vector<double> tan_phi; std::vector<int> shift;               // [num_phi]
    std::vector<double> sR, C_D, rs_D;                                 // [pano_width * 9], [pano_width * 3], [pano_width * num_phi * 3]
};

inline void pano_theta_table(const PanoParams& P, int pano_width, PanoThetaTable& T) {
    using namespace pano_detail;
    const double up[3] = {0, 1, 0}, synth_t[3] = {0, 0, -P.synth_radius};
    const double theta_step = (M_PI - (-M_PI)) / (pano_width - 1);
    T.tan_phi.resize((size_t)P.num_phi); T.shift.resize((size_t)P.num_phi);
    for (int p = 0; p < P.num_phi; p++) { const double phi = pano_phi(P, p); T.tan_phi[(size_t)p] = std::tan(phi); T.shift[(size_t)p] = (int)std::round(phi / theta_step); }
    T.sR.resize((size_t)pano_width * 9); T.C_D.resize((size_t)pano_width * 3); T.rs_D.resize((size_t)pano_width * (size_t)P.num_phi * 3);
    for (int th = 0; th < pano_width; th++) {
        const double theta = -M_PI + th * theta_step;
        double* sR = &T.sR[(size_t)th * 9];
        so3exp_y(theta, sR); center(sR, synth_t, &T.C_D[(size_t)th * 3]);
        for (int p = 0; p < P.num_phi; p++) {
            const double d[3] = {T.tan_phi[(size_t)p] - synth_t[0], 0.0 - synth_t[1], 1.0 - synth_t[2]};
            double r_D[3]; mul_Rt(sR, d, r_D); project(r_D, up, &T.rs_D[((size_t)th * (size_t)P.num_phi + (size_t)p) * 3]);
        }
    }
}

// The jobs of the pairs [k0, k1), in the reference's order.  R row-major [n * 9], t [n * 3].
// The three tests of :587-592 are made on the angles, as the reference makes them, but only where they can pass: atan2(y, x) is below pi/2 in magnitude only for
// x > 0, and two angles have a negative product only when their y are non-zero with opposite signs (y = +-0 gives +-0 or +-pi).  Both are read off the very
// values that go into atan2, so skipping the other (pair, thetanum, phinum), all but a fraction of a percent, changes no result.
inline void pano_plan_pairs(const PanoParams& P, int n, const double* R, const double* t, double focal, double cy, int height, int pano_width, const PanoThetaTable& T,
                            int k0, int k1, std::vector<PanoJob>& out) {
    using namespace pano_detail;
    const double up[3] = {0, 1, 0};
    const double synth_focal = focal * P.synth_focal_factor;
    for (int k = k0; k < k1; k++) {
        const int l = k, r = (k + 1) % n;
        double C_L[3], C_R[3]; center(R + 9 * (size_t)l, t + 3 * (size_t)l, C_L); center(R + 9 * (size_t)r, t + 3 * (size_t)r, C_R);
        for (int th = 0; th < pano_width; th++) {
            const double* C_D = &T.C_D[(size_t)th * 3];
            const double r_L[3] = {C_L[0] - C_D[0], C_L[1] - C_D[1], C_L[2] - C_D[2]}, r_R[3] = {C_R[0] - C_D[0], C_R[1] - C_D[1], C_R[2] - C_D[2]};
            double rs_L[3], rs_R[3]; project(r_L, up, rs_L); project(r_R, up, rs_R);
            for (int p = 0; p < P.num_phi; p++) {
                const double* rs_D = &T.rs_D[((size_t)th * (size_t)P.num_phi + (size_t)p) * 3];
                double cL[3], cR[3]; cross(rs_L, rs_D, cL); cross(rs_R, rs_D, cR);
                const double yL = dot3(cL, up), xL = dot3(rs_L, rs_D), yR = dot3(cR, up), xR = dot3(rs_R, rs_D);
                if (!(xL > 0 && xR > 0 && ((yL > 0 && yR < 0) || (yL < 0 && yR > 0)))) continue;
                const double angle_LD = std::atan2(yL, xL), angle_RD = std::atan2(yR, xR);
                if (!(angle_LD * angle_RD < 0)) continue;
                if (std::fabs(angle_LD) >= M_PI / 2) continue;
                if (std::fabs(angle_RD) >= M_PI / 2) continue;
                const double angle_LR = signed_angle_between(rs_L, rs_R, up);
                PanoJob j;
                j.pair = k; j.theta = th; j.phi = p;
                j.alpha = std::fabs(angle_LD) / std::fabs(angle_LR);
                int col = (th + T.shift[(size_t)p]) % pano_width; if (col < 0) col += pano_width;
                j.col = col; j.tan_phi = T.tan_phi[(size_t)p];
                for (int i = 0; i < 9; i++) j.synth_R[i] = T.sR[(size_t)th * 9 + i];
                const PanoRowConsts c = pano_row_consts(j.tan_phi, j.synth_R, P.depth, P.synth_radius);
                j.ok = depth_positive_on_every_row(c, R + 9 * (size_t)l, t + 3 * (size_t)l, cy, synth_focal, P.depth, height) &&
                       depth_positive_on_every_row(c, R + 9 * (size_t)r, t + 3 * (size_t)r, cy, synth_focal, P.depth, height) ? 1 : 0;
                out.push_back(j);
            }
        }
    }
}

// Pairs are independent, so they are planned on up to `threads` threads (started and joined here) and concatenated in pair order.
inline void pano_plan(const PanoParams& P, int n, const double* R, const double* t, double focal, double cy, int height, int pano_width, int threads, PanoPlan& plan) {
    const int pairs = pano_num_pairs(n, P.is_loop);
    plan.num_pairs = pairs; plan.jobs.clear();
    plan.owner.assign((size_t)P.num_phi * (size_t)pano_width, -1); plan.owner_job.assign((size_t)P.num_phi * (size_t)pano_width, -1);
    PanoThetaTable table; pano_theta_table(P, pano_width, table);
    const int T = std::max(1, std::min(threads, pairs / 4));
    if (T <= 1) {
        pano_plan_pairs(P, n, R, t, focal, cy, height, pano_width, table, 0, pairs, plan.jobs);
    } else {
        std::vector<std::vector<PanoJob>> part((size_t)T); std::vector<std::thread> th;
        for (int i = 0; i < T; i++)
            th.emplace_back([&, i]() { pano_plan_pairs(P, n, R, t, focal, cy, height, pano_width, table, (int)((int64_t)pairs * i / T), (int)((int64_t)pairs * (i + 1) / T), part[(size_t)i]); });
        for (auto& x : th) x.join();
        for (auto& v : part) plan.jobs.insert(plan.jobs.end(), v.begin(), v.end());
    }
    for (size_t j = 0; j < plan.jobs.size(); j++) {                  // ascending pair: the last ok writer stays
        const PanoJob& J = plan.jobs[j];
        if (!J.ok) continue;
        const size_t o = (size_t)J.phi * (size_t)pano_width + (size_t)J.col;
        plan.owner[o] = J.pair; plan.owner_job[o] = (int32_t)j;
    }
}

inline const char* pano_check_params(const PanoParams& P, int n, const double* R, const double* t, double focal, int width, int height, int pano_width) {
    if (n < 0) return "n is negative";
    if (n > 0 && (!R || !t)) return "R or t is null";
    if (P.num_phi < 1) return "num_phi < 1";
    if (pano_width < 2) return "pano_width < 2";
    if (width < 1 || height < 1) return "width or height < 1";
    if (!(focal > 0.0) || !std::isfinite(focal)) return "focal is not positive";
    if (!(P.synth_focal_factor > 0.0) || !std::isfinite(P.depth) || !std::isfinite(P.synth_radius) || !std::isfinite(P.phi_step_deg)) return "bad options";
    if ((int64_t)P.num_phi * (int64_t)pano_width > (int64_t)1 << 30) return "num_phi * pano_width is too large";
    return nullptr;
}

}  // namespace ssfm
