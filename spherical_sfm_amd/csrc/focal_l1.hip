// spherical_sfm_amd -- robust focal search over a view graph (include/ssfm.h: ssfm_focal_search_l1): per trial focal the matches are re-derived as in
// ssfm_focal_search_graph, the rotations are solved by the L1 iteratively reweighted least squares of ssfm_rot_l1_init, and the trial is judged by sum |v_e|.
//
//   k_focal_l1_start    phase A, one workgroup per trial: k_focal_trials_graph (view_graph.hip) up to the chained rotations, through the same device functions in the
//                       same order -- transform every edge, store so3ln(so3exp(r)), identity for the root and the unreached cameras, the tree level by level.
//   k_focal_trials_l1   phases B and C, one workgroup of 256 lanes per trial, the whole IRLS loop inside the launch: the barriers of the workgroup stand where
//                       ssfm_rot_l1_init has ~10^3 launches per solve.  Per outer iteration a lane per edge writes the record (w, w v), a lane per node walks its
//                       incident list in adjacency order for L_ii, g_i and the CG start, CG runs with the matvec by gathers, a lane per node applies the update.
//                       Every decision (column stop, cap, step test) is taken from sums that all lanes read from LDS after a barrier: the workgroup never diverges.
//                       Phase C: the residual pass, sum |v_e|, the iteration count.
//   k_focal_l1_get_cost get_cost at the returned rotations as k_focal_trials_graph's last loop computes it.
// Three launches per slab, not one: with all phases in one kernel the compiler puts 80 B per lane into scratch (the figure of k_focal_trials_graph, which has
// phase A and get_cost in one kernel); apart, none of the three uses scratch (scripts/kernel_resources.py), and the CG loop is the one that must not.
// The CG vectors (x, r, z, p, q: 15 n doubles), the diagonal (n) and the edge records (4 E) live in dynamic LDS when they fit beside the reductions, in a
// per-trial global slice otherwise.  The kernel reaches them through one generic pointer, so both placements execute the same instructions on the same values
// and give the same bits.  SSFM_FOCAL_L1_FORCE_GLOBAL=1 (read at call time) forces the global slice.
//
// REPRODUCIBLE: no floating-point atomic.  A lane adds its strided items in ascending order, a wave folds by the xor butterfly (wave_sum), the four wave partials
// add in wave order.  The order is fixed by (n, E, adjacency) alone, and a workgroup sees nothing of another trial: a trial's outputs do not depend on its
// position, on num_trials, on the slab it falls into or on the run.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "ransac_device.h"
#include "rot_l1_host.h"

namespace ssfm {

static constexpr int kFl1Threads = 256;
static constexpr size_t kFl1LdsBudget = 156 * 1024;      // static + dynamic LDS of one workgroup (five-point section; the CU has 160 KiB)
static constexpr size_t kFl1LdsStatic = 512;             // the reduction buffers below (384 B), rounded up

__global__ void __launch_bounds__(kFl1Threads)
k_focal_l1_start(int n, int E, int num_levels, const int* __restrict__ level_ptr, const int* __restrict__ tree_node, const int* __restrict__ tree_parent,
                 const int* __restrict__ tree_edge, const int* __restrict__ tree_rev, const double* __restrict__ Es /*[E*9] row-major*/, int inward,
                 double focal_guess, const double* __restrict__ focals, double* __restrict__ rnew_all /*[trials*E*3]*/,
                 double* __restrict__ rot_all /*[trials*n*9] row-major*/, double* __restrict__ scale_all /*[trials]*/) {
    __shared__ double red[4];
    const int trial = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const double f = focals[trial], tf = f / focal_guess;
    double* rnew = rnew_all + (size_t)trial * E * 3; double* rot = rot_all + (size_t)trial * n * 9;
    double mx = 0.0;
    for (int e = tid; e < E; e += nt) {
        double En[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) En[3 * i + j] = Es[9 * (size_t)e + 3 * i + j] * ((i < 2) ? tf : 1.0) * ((j < 2) ? tf : 1.0);
        double r[3]; decompose_E_dev(En, inward != 0, r);
        // the reference stores so3exp(r_new) and get_cost takes so3ln of it again
        double Rm[9], rr[3]; so3exp(r, Rm); so3ln(Rm, rr);
        double* o = rnew + 3 * (size_t)e;                                            // E may reach 2^30: 3 e does not fit an int
        o[0] = rr[0]; o[1] = rr[1]; o[2] = rr[2];
        mx = fmax(mx, norm3(rr));
    }
    for (int i = tid; i < n; i += nt) { double* dst = rot + 9 * (size_t)i; for (int k = 0; k < 9; k++) dst[k] = (k % 4 == 0) ? 1.0 : 0.0; }     // the root and every unreached camera
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) { double m = 0; for (int w = 0; w < (nt >> 6); w++) m = fmax(m, red[w]); scale_all[trial] = 1.0 / m; }
    // level by level: a node's parent was written one level earlier (global writes of this block are visible to it after the barrier)
    for (int l = 1; l < num_levels; l++) {
        for (int k = level_ptr[l] + tid; k < level_ptr[l + 1]; k += nt) {
            const int e = tree_edge[k];
            double Rm[9], Rp[9], Rn[9];
            so3exp(rnew + 3 * (size_t)e, Rm);
            for (int q = 0; q < 9; q++) Rp[q] = rot[9 * (size_t)tree_parent[k] + q];
            if (tree_rev[k]) mat3_mul_at(Rm, Rp, Rn); else mat3_mul(Rm, Rp, Rn);
            double* dst = rot + 9 * (size_t)tree_node[k];
            for (int q = 0; q < 9; q++) dst[q] = Rn[q];
        }
        __syncthreads();
    }
}

// Workgroup sums of N values; every lane leaves with the same N sums.  red alternates between its two halves: a lane that writes a half again has passed the
// barrier of the reduction in between, which every reader of that half reached after its reads -- one barrier per reduction.  MAX: maxima instead of sums.
template <int N, bool MAX>
__device__ __forceinline__ void fl1_reduce(double (&v)[N], double (*red)[4][6], int& par) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < N; c++) {
        const double s = MAX ? wave_max(v[c]) : wave_sum(v[c]);
        if (lane == 0) red[par][w][c] = s;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; c++)
        v[c] = MAX ? fmax(fmax(red[par][0][c], red[par][1][c]), fmax(red[par][2][c], red[par][3][c])) : ((red[par][0][c] + red[par][1][c]) + red[par][2][c]) + red[par][3][c];
    par ^= 1;
}

// v_e = so3ln(R_b^T R_e R_a) of every edge, R_e = so3exp(rnew_e).  FINAL = false: the records (w, w v).  FINAL = true: the residuals; returns the lane's share of sum |v_e|.
template <bool FINAL>
__device__ __forceinline__ double fl1_edges(int E, const int* __restrict__ e0, const int* __restrict__ e1, const int* __restrict__ reached,
                                            const double* __restrict__ rnew, const double* rot, double floor_w, double* rec, double* __restrict__ residual) {
    double c = 0.0;
    for (int e = threadIdx.x; e < E; e += kFl1Threads) {
        const int a = e0[e], b = e1[e];
        const bool used = a != b && reached[a] && reached[b];
        double v[3] = {0.0, 0.0, 0.0}, w = 0.0, nrm = 0.0;
        if (used) {
            double Re[9], Ra[9], Rb[9], T[9], D[9];
            so3exp(rnew + 3 * (size_t)e, Re);
#pragma unroll
            for (int q = 0; q < 9; q++) { Ra[q] = rot[9 * (size_t)a + q]; Rb[q] = rot[9 * (size_t)b + q]; }
            mat3_mul(Re, Ra, T); mat3_mul_at(Rb, T, D);
            so3ln(D, v);
            nrm = norm3(v);
            w = 1.0 / fmax(nrm, floor_w);
        }
        if (FINAL) { residual[e] = used ? nrm : -1.0; c += nrm; }
        else { double* o = rec + 4 * (size_t)e; o[0] = w; o[1] = w * v[0]; o[2] = w * v[1]; o[3] = w * v[2]; }
    }
    return c;
}

// work_all == nullptr: Lii, x, r, z, p, q and the records in dynamic LDS ((16 n + 4 E) doubles); otherwise trial t owns work_all + t * work_stride.
__global__ void __launch_bounds__(kFl1Threads)
k_focal_trials_l1(int n, int E, int edges_used, const int* __restrict__ e0, const int* __restrict__ e1, const int* __restrict__ reached,
                  const int* __restrict__ free_node, const int* __restrict__ adj_ptr, const int* __restrict__ adj_nb, const unsigned* __restrict__ adj_es,
                  const double* __restrict__ rnew_all, double* rot_all, double* work_all, size_t work_stride,
                  double* __restrict__ res_all /*[trials*E]*/, int max_iterations, double step_tolerance, double floor_w, double tol2, int cap,
                  double* __restrict__ costs, int* __restrict__ iterations) {
    extern __shared__ double s_work[];
    __shared__ double red[2][4][6];
    const int trial = blockIdx.x, tid = threadIdx.x;
    const double* rnew = rnew_all + (size_t)trial * E * 3; double* rot = rot_all + (size_t)trial * n * 9; double* residual = res_all + (size_t)trial * E;
    double* W = work_all ? work_all + (size_t)trial * work_stride : s_work;
    double* Lii = W; double* x = Lii + n; double* r = x + 3 * (size_t)n; double* z = r + 3 * (size_t)n; double* p = z + 3 * (size_t)n; double* q = p + 3 * (size_t)n;
    double* rec = q + 3 * (size_t)n;
    int par = 0, outer = 0;
    if (edges_used > 0) {                                                            // a root without used edges: identities, 0 iterations (ssfm_rot_l1_init)
        for (int k = 1; k <= max_iterations; k++) {
            fl1_edges<false>(E, e0, e1, reached, rnew, rot, floor_w, rec, nullptr);
            __syncthreads();
            // the diagonal, the right-hand side and the CG start; the root and the unreached cameras are rows with L_ii = 1 and zeros
            double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                           // r.z and g.g per column
            for (int i = tid; i < n; i += kFl1Threads) {
                double sw = 0.0, g[3] = {0.0, 0.0, 0.0};
                if (free_node[i]) {
                    for (int a = adj_ptr[i]; a < adj_ptr[i + 1]; a++) {
                        const unsigned es = adj_es[a];
                        const double* o = rec + 4 * (size_t)(es >> 1);
                        const double sgn = (es & 1u) ? 1.0 : -1.0;
                        sw += o[0]; g[0] += sgn * o[1]; g[1] += sgn * o[2]; g[2] += sgn * o[3];
                    }
                }
                const double d = free_node[i] ? sw : 1.0;                            // a free node has an edge to its tree parent: sw > 0
                Lii[i] = d;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double zc = g[c] / d;
                    x[3 * i + c] = 0.0; r[3 * i + c] = g[c]; z[3 * i + c] = zc; p[3 * i + c] = zc; q[3 * i + c] = 0.0;
                    s6[c] += g[c] * zc; s6[3 + c] += g[c] * g[c];
                }
            }
            fl1_reduce<6, false>(s6, red, par);                                      // its barrier also publishes p to the gathers below
            double rz[3], gg[3]; int flag[3];
#pragma unroll
            for (int c = 0; c < 3; c++) { rz[c] = s6[c]; gg[c] = s6[3 + c]; flag[c] = gg[c] <= tol2 * gg[c] ? 1 : 0; }     // r = g: a zero column is done at once
            int iters = 0;
            bool done = (flag[0] && flag[1] && flag[2]) || cap <= 0;
            while (!done) {                                                          // uniform: every lane holds the same sums
                double pq[3] = {0.0, 0.0, 0.0};
                for (int i = tid; i < n; i += kFl1Threads) {
                    if (!free_node[i]) continue;
                    double a3[3] = {0.0, 0.0, 0.0};
                    for (int a = adj_ptr[i]; a < adj_ptr[i + 1]; a++) {
                        const double w = rec[4 * (size_t)(adj_es[a] >> 1)];
                        const double* pn = p + 3 * (size_t)adj_nb[a];
                        a3[0] += w * pn[0]; a3[1] += w * pn[1]; a3[2] += w * pn[2];
                    }
#pragma unroll
                    for (int c = 0; c < 3; c++) { const double pc = p[3 * i + c], qc = Lii[i] * pc - a3[c]; q[3 * i + c] = qc; pq[c] += pc * qc; }
                }
                fl1_reduce<3, false>(pq, red, par);
                double alpha[3]; int act[3];
#pragma unroll
                for (int c = 0; c < 3; c++) { act[c] = flag[c] ? 0 : 1; alpha[c] = act[c] ? rz[c] / pq[c] : 0.0; }
                double t6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                       // r.z and r.r per column
                for (int i = tid; i < n; i += kFl1Threads) {
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        if (!act[c]) continue;
                        const int j = 3 * i + c;
                        const double xj = x[j] + alpha[c] * p[j], rj = r[j] - alpha[c] * q[j], zj = rj / Lii[i];
                        x[j] = xj; r[j] = rj; z[j] = zj;
                        t6[c] += rj * zj; t6[3 + c] += rj * rj;
                    }
                }
                fl1_reduce<6, false>(t6, red, par);                                  // every gather of p above lies before this barrier
                double beta[3];
#pragma unroll
                for (int c = 0; c < 3; c++) beta[c] = act[c] ? t6[c] / rz[c] : 0.0;
                for (int i = tid; i < n; i += kFl1Threads) {
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        if (!act[c]) continue;
                        const int j = 3 * i + c;
                        p[j] = z[j] + beta[c] * p[j];
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; c++)
                    if (act[c]) { rz[c] = t6[c]; flag[c] = t6[3 + c] <= tol2 * gg[c] ? 1 : 0; }
                iters++;
                done = (flag[0] && flag[1] && flag[2]) || iters >= cap;
                __syncthreads();                                                     // the new p before the next gathers
            }
            // R_i <- R_i so3exp(x_i), step = max |x_i|
            double m1[1] = {0.0};
            for (int i = tid; i < n; i += kFl1Threads) {
                if (!free_node[i]) continue;
                double R[9], dR[9], Rn[9];
                const double xi[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
#pragma unroll
                for (int c = 0; c < 9; c++) R[c] = rot[9 * (size_t)i + c];
                so3exp(xi, dR); mat3_mul(R, dR, Rn);
#pragma unroll
                for (int c = 0; c < 9; c++) rot[9 * (size_t)i + c] = Rn[c];
                m1[0] = fmax(m1[0], norm3(xi));
            }
            fl1_reduce<1, true>(m1, red, par);                                       // its barrier publishes the rotations to the next edge pass
            outer = k;
            if (m1[0] < step_tolerance) break;                                       // uniform
        }
    }
    // phase C: the residuals and sum |v_e| at the returned rotations
    double c1[1];
    c1[0] = fl1_edges<true>(E, e0, e1, reached, rnew, rot, floor_w, nullptr, residual);
    fl1_reduce<1, false>(c1, red, par);
    if (tid == 0) { costs[trial] = c1[0]; iterations[trial] = outer; }
}

// get_cost at the rotations and the matches of every trial: the last loop of k_focal_trials_graph, the same device functions in the same order.
// A launch of its own: see the head of the file.
__global__ void __launch_bounds__(kFl1Threads)
k_focal_l1_get_cost(int n, int E, const int* __restrict__ e0, const int* __restrict__ e1, const double* __restrict__ rnew_all, const double* __restrict__ rot_all,
                    const double* __restrict__ scale_all, double* __restrict__ x_all /*[trials*n*3]*/, double* __restrict__ get_costs) {
    __shared__ double red[4];
    const int trial = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const double* rnew = rnew_all + (size_t)trial * E * 3; const double* rot = rot_all + (size_t)trial * n * 9; double* x = x_all + (size_t)trial * n * 3;
    for (int i = tid; i < n; i += nt) so3ln(rot + 9 * (size_t)i, x + 3 * i);
    __syncthreads();
    const double scale = scale_all[trial];
    double c = 0.0;
    for (int e = tid; e < E; e += nt) {
        double Rm[9], R0[9], R1[9], A[9], C[9], res[3];
        angle_axis_to_matrix(rnew + 3 * (size_t)e, Rm); angle_axis_to_matrix(x + 3 * (size_t)e0[e], R0); angle_axis_to_matrix(x + 3 * (size_t)e1[e], R1);
        mat3_mul_bt(R1, R0, A); mat3_mul_bt(A, Rm, C);
        matrix_to_angle_axis(C, res);
        const double s2 = scale * scale * (res[0] * res[0] + res[1] * res[1] + res[2] * res[2]);
        double rho0, rho1; robust_loss(2, 0.03, s2, rho0, rho1);
        c += 0.5 * rho0;
    }
    c = wave_sum(c);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) { double t = 0; for (int w = 0; w < (nt >> 6); w++) t += red[w]; get_costs[trial] = t; }
}

}  // namespace ssfm
using namespace ssfm;

// The per-trial workspace of one slab (rnew 3 E, residuals E, rotations 9 n, get_cost's angle-axis 3 n and, in the global placement, the vectors and the records)
// stays within this bound: all pairs of 500 cameras x 1024 trials would be 8 GB unslabbed.  A slab should still fill the device -- 256 compute units, a few
// workgroups each -- so the bound is 1 GiB and not the 64 MB of the record slabs of view_graph.hip, and the trials are split evenly over the slabs.
// SSFM_FOCAL_L1_SLAB_TRIALS (read at every call, like SSFM_TRIPLET_SLAB_RECORDS) overrides the trial count of a slab, so that a small problem can walk the
// multi-slab path.
static const size_t kFl1SlabBytes = (size_t)1 << 30;
static bool fl1_force_global() { const char* e = getenv("SSFM_FOCAL_L1_FORCE_GLOBAL"); return e && atoi(e) != 0; }       // read at call time (tests)

// a failed HIP call: wait for what is in flight, give the temporaries back (ssfm_ctx.h: the pool's rule), report
#define FL1_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipStreamSynchronize(st); release(); return fail(ctx, SSFM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)

extern "C" void ssfm_focal_l1_default_options(ssfm_rot_l1_options* o) {
    if (!o) return;
    ssfm_rot_l1_default_options(o);
    o->max_iterations = 10;
}

extern "C" int ssfm_focal_search_l1(ssfm_ctx* ctx, int32_t n, int32_t E, const int32_t* index0, const int32_t* index1, const double* rel_rotations, int32_t inward,
                                    double focal_guess, int32_t num_trials, const double* focals, int32_t root, const ssfm_rot_l1_options* opt, double* costs,
                                    double* get_costs, int32_t* iterations, int32_t* best_trial, double* rotations_best, double* rel_rotations_best,
                                    double* residual_best, double* kernel_ms) {
    const std::string who = "ssfm_focal_search_l1: ";
    // what ssfm_focal_search_graph refuses, then what ssfm_rot_l1_init refuses, in its order (options, indices, root); the context last.  Nothing is launched before.
    if (n <= 0 || n > (1 << 29) || E <= 0 || E > (1 << 30) || num_trials <= 0 || !index0 || !index1 || !rel_rotations || !focals)
        return fail(ctx, SSFM_ERR_INVALID, who + "bad arguments");
    // rot_l1_check only tests its last two arguments (ssfm_rot_l1_init's outputs, which this call does not have) against NULL and never dereferences them:
    // any non-null pointers pass.  Should it ever read them, this call needs a check of its own.
    ssfm_rot_l1_summary not_read;
    if (const char* why = rot_l1_check(n, E, index0, index1, rel_rotations, root, opt, /* rotations_out, NULL test only */ rel_rotations, &not_read))
        return fail(ctx, SSFM_ERR_INVALID, who + why);
    if (!ctx) return fail(ctx, SSFM_ERR_INVALID, who + "ctx is null");
    if (ctx->collective) return fail(ctx, SSFM_ERR_INVALID, who + "the context carries a communicator; this call is single-GPU");
    ssfm_rot_l1_options O;
    if (opt) O = *opt; else ssfm_focal_l1_default_options(&O);
    // the tree with its levels and the node-major adjacency: neither depends on the focal
    std::vector<int> t_node((size_t)n), t_parent((size_t)n), t_edge((size_t)n), level_ptr((size_t)n + 1); std::vector<uint8_t> t_rev8((size_t)n);
    int32_t num_reached = 0, levels = 0;
    RotL1Graph G;
    if (view_graph_tree(n, E, index0, index1, root, &num_reached, t_node.data(), t_parent.data(), t_edge.data(), t_rev8.data(), &levels, level_ptr.data()) != 0 ||
        !rot_l1_graph(n, E, index0, index1, root, G))
        return fail(ctx, SSFM_ERR_INVALID, who + "root or camera index out of range");
    std::vector<int> t_rev(t_rev8.begin(), t_rev8.end());
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // Es[i] = make_spherical_essential_matrix(R_i, inward), row-major for the device: as ssfm_focal_search_graph forms it
    std::vector<double> Es((size_t)9 * E); std::vector<int> e0(index0, index0 + E), e1(index1, index1 + E);
    for (int e = 0; e < E; e++) {
        double Rm[9]; cm_to_rm(rel_rotations + 9 * (size_t)e, Rm);
        double t[3] = {Rm[2], Rm[5], Rm[8] - 1.0}; if (inward) { t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2]; }
        double* Em = &Es[9 * (size_t)e];
        for (int j = 0; j < 3; j++) { Em[j] = t[1] * Rm[6 + j] - t[2] * Rm[3 + j]; Em[3 + j] = t[2] * Rm[j] - t[0] * Rm[6 + j]; Em[6 + j] = t[0] * Rm[3 + j] - t[1] * Rm[j]; }
    }
    // placement and slab size
    const size_t work_doubles = (size_t)16 * n + (size_t)4 * E;
    const bool in_lds = !fl1_force_global() && work_doubles * sizeof(double) + kFl1LdsStatic <= kFl1LdsBudget;
    const size_t lds = in_lds ? work_doubles * sizeof(double) : 0;
    const size_t per_trial = ((size_t)3 * E + (size_t)E + (size_t)12 * n + (in_lds ? 0 : work_doubles)) * sizeof(double);
    long long slab_trials = (long long)std::max<size_t>(1, kFl1SlabBytes / per_trial);
    if (slab_trials < num_trials) { const long long slabs = (num_trials + slab_trials - 1) / slab_trials; slab_trials = (num_trials + slabs - 1) / slabs; }   // evenly
    if (const char* e = getenv("SSFM_FOCAL_L1_SLAB_TRIALS")) slab_trials = std::max<long long>(1, atoll(e));
    const int S = (int)std::min<long long>(slab_trials, num_trials);
    const int cap = O.pcg_max_iterations > 0 ? O.pcg_max_iterations : (int)std::min<long long>(4LL * G.num_free, 0x7fffffffLL);
    const double tol2 = O.pcg_tolerance * O.pcg_tolerance;

    DevBuf<double> dEs, dF, dRnew, dRot, dScale, dWork, dRes, dC, dGC, dX; DevBuf<int> de0, de1, dlv, dtn, dtp, dte, dtr, dReached, dFree, dAptr, dAnb, dIt; DevBuf<unsigned> dAes;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    auto release = [&]() {
        dEs.free(); dF.free(); dRnew.free(); dRot.free(); dScale.free(); dWork.free(); dRes.free(); dC.free(); dGC.free(); dX.free(); de0.free(); de1.free(); dlv.free(); dtn.free();
        dtp.free(); dte.free(); dtr.free(); dReached.free(); dFree.free(); dAptr.free(); dAnb.free(); dIt.free(); dAes.free();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        ev0 = ev1 = nullptr;
    };
    FL1_CHECK(hipEventCreate(&ev0)); FL1_CHECK(hipEventCreate(&ev1));
    if (lds > 48 * 1024) FL1_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_focal_trials_l1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    std::vector<double> fv(focals, focals + num_trials);
    FL1_CHECK(upload(dEs, Es, st)); FL1_CHECK(upload(dF, fv, st)); FL1_CHECK(upload(de0, e0, st)); FL1_CHECK(upload(de1, e1, st));
    FL1_CHECK(upload(dlv, level_ptr, st)); FL1_CHECK(upload(dtn, t_node, st)); FL1_CHECK(upload(dtp, t_parent, st)); FL1_CHECK(upload(dte, t_edge, st));
    FL1_CHECK(upload(dtr, t_rev, st)); FL1_CHECK(upload(dReached, G.reached, st)); FL1_CHECK(upload(dFree, G.free_node, st));
    FL1_CHECK(upload(dAptr, G.adj_ptr, st)); FL1_CHECK(upload(dAnb, G.adj_nb, st)); FL1_CHECK(upload(dAes, G.adj_es, st));
    FL1_CHECK(dRnew.alloc((size_t)S * E * 3)); FL1_CHECK(dRot.alloc((size_t)S * n * 9)); FL1_CHECK(dScale.alloc(S)); FL1_CHECK(dRes.alloc((size_t)S * E));
    FL1_CHECK(dC.alloc(S)); FL1_CHECK(dGC.alloc(S)); FL1_CHECK(dIt.alloc(S)); FL1_CHECK(dX.alloc((size_t)S * n * 3));
    if (!in_lds) FL1_CHECK(dWork.alloc((size_t)S * work_doubles));

    std::vector<double> hc((size_t)num_trials), hg((size_t)num_trials), h_rot((size_t)n * 9), h_rnew((size_t)E * 3), h_res((size_t)E); std::vector<int> hi((size_t)num_trials);
    int best = -1; double ms_total = 0.0;
    for (int t0 = 0; t0 < num_trials; t0 += S) {
        const int T = std::min(S, num_trials - t0);
        FL1_CHECK(hipEventRecord(ev0, st));
        hipLaunchKernelGGL(k_focal_l1_start, dim3(T), dim3(kFl1Threads), 0, st, n, E, levels, dlv.p, dtn.p, dtp.p, dte.p, dtr.p, dEs.p, inward, focal_guess, dF.p + t0,
                           dRnew.p, dRot.p, dScale.p);
        FL1_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_focal_trials_l1, dim3(T), dim3(kFl1Threads), lds, st, n, E, G.num_edges_used, de0.p, de1.p, dReached.p, dFree.p, dAptr.p, dAnb.p, dAes.p,
                           dRnew.p, dRot.p, in_lds ? nullptr : dWork.p, work_doubles, dRes.p, O.max_iterations, O.step_tolerance, O.weight_floor, tol2, cap, dC.p, dIt.p);
        FL1_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_focal_l1_get_cost, dim3(T), dim3(kFl1Threads), 0, st, n, E, de0.p, de1.p, dRnew.p, dRot.p, dScale.p, dX.p, dGC.p);
        FL1_CHECK(hipGetLastError());
        FL1_CHECK(hipEventRecord(ev1, st));
        FL1_CHECK(hipMemcpyAsync(hc.data() + t0, dC.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, st));
        FL1_CHECK(hipMemcpyAsync(hg.data() + t0, dGC.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, st));
        FL1_CHECK(hipMemcpyAsync(hi.data() + t0, dIt.p, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, st));
        FL1_CHECK(hipStreamSynchronize(st));
        float ms = 0.f;
        FL1_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
        ms_total += ms;
        const int prev = best;                                                                              // strict <, first minimum, across the slabs in order
        for (int t = t0; t < t0 + T; t++) if (best < 0 || hc[(size_t)t] < hc[(size_t)best]) best = t;
        if (best != prev) {                                                                                 // the slab's buffers are reused: take the best trial's slices now
            const size_t k = (size_t)(best - t0);
            FL1_CHECK(hipMemcpyAsync(h_rot.data(), dRot.p + k * n * 9, h_rot.size() * sizeof(double), hipMemcpyDeviceToHost, st));
            FL1_CHECK(hipMemcpyAsync(h_rnew.data(), dRnew.p + k * E * 3, h_rnew.size() * sizeof(double), hipMemcpyDeviceToHost, st));
            FL1_CHECK(hipMemcpyAsync(h_res.data(), dRes.p + k * E, h_res.size() * sizeof(double), hipMemcpyDeviceToHost, st));
            FL1_CHECK(hipStreamSynchronize(st));
        }
    }
    release();                                                                                               // the stream has drained
    if (costs) std::memcpy(costs, hc.data(), hc.size() * sizeof(double));
    if (get_costs) std::memcpy(get_costs, hg.data(), hg.size() * sizeof(double));
    if (iterations) std::memcpy(iterations, hi.data(), hi.size() * sizeof(int));
    if (best_trial) *best_trial = best;
    if (rotations_best) for (int i = 0; i < n; i++) rm_to_cm(&h_rot[9 * (size_t)i], rotations_best + 9 * (size_t)i);
    if (rel_rotations_best)                                    // the matches as transform_image_matches leaves them at the best focal
        for (int e = 0; e < E; e++) { double Rm[9]; so3exp(&h_rnew[3 * (size_t)e], Rm); rm_to_cm(Rm, rel_rotations_best + 9 * (size_t)e); }
    if (residual_best) std::memcpy(residual_best, h_res.data(), h_res.size() * sizeof(double));
    if (kernel_ms) *kernel_ms = ms_total;
    return SSFM_OK;
}
