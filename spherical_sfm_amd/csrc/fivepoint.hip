// spherical_sfm_amd -- general relative pose: LocallyOptimizedMSAC over the five-point (Stewenius) estimator with the reference's own sample
// trace, one workgroup per image pair.
//
//   estimate_pairwise_five_point                                                            examples/spherical_sfm_tools.cpp:433-573
//   ransac_lib::LocallyOptimizedMSAC<Matrix3d, ..., SteweniusEstimator>::EstimateModel       include/RansacLib/ransac.h:128-275
//   SteweniusEstimator / FivePointEstimator / PoseFromEssentialMatrix                        evaluation/five_point/*.cpp
//
// k_lomsac5_trace runs the control flow of lomsac_trace.h (the one k_lomsac_trace of lomsac.hip runs) for a minimal sample of five.  What the
// estimator changes:
//   * up to ten candidate models per minimal sample, scored in two sweeps of five over the rays;
//   * SteweniusEstimator::NonMinimalSolver returns 0 and LeastSquares is empty, so LocalOptimization and the final least squares change no
//     model and no score: LocalOptimization is kept for what it still does -- it counts in stats and its LeastSquaresFit shuffles the inlier
//     list, which advances the local-optimisation stream -- and the final least squares, which re-scores the unchanged model, is dropped;
//     with it goes the second model: best_model and best_minimal_model are always the same matrix here (LO_CHANGES_MODEL = false).
//   * the tail is estimate_pairwise_five_point's: inlier flags by the epipolar-line residual, acceptance, PoseFromEssentialMatrix.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "fivepoint_device.h"
#include "lomsac_trace.h"

namespace ssfm {

constexpr int L5_T = LO_T;                     // threads per pair
constexpr int L5_RAY_DOUBLES = 5;              // LDS per ray: u0/u2, u1/u2, v0, v1, v2
constexpr size_t L5_LDS_FIXED = lo_lds_fixed(5);   // both generator states + the FIFO
constexpr size_t L5_LDS_BUDGET = 156 * 1024;   // static + dynamic LDS of one workgroup (the CU has 160 KiB)

using Lo5Opts = LoTraceOpts;                   // this estimator has no options of its own
struct Lo5Shared {                             // static LDS of the trace kernel
    double score[L5_T]; double E[9];
    int sample[5 * L5_T]; int nm[L5_T]; int votes[4]; int cnt; int flag;
};
constexpr int l5_max_lds_rays() { return (int)((L5_LDS_BUDGET - sizeof(Lo5Shared) - L5_LDS_FIXED) / (L5_RAY_DOUBLES * sizeof(double))); }

// number of rays with residual(E) < thresh: integer count, every thread returns it
template <bool RAYS_LDS>
__device__ int l5_count_inliers(const double* E, const FpRays<RAYS_LDS>& rays, int n, double thresh, int* s_cnt) {
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) mine += (rays.residual(E, i) < thresh) ? 1 : 0;
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    if (mine) atomicAdd(s_cnt, mine);
    __syncthreads();
    const int r = *s_cnt;
    __syncthreads();
    return r;
}

// LocalOptimization (ransac.h:341-407) over SteweniusEstimator with num_lo_steps_ = 0: LeastSquaresFit's shuffle of the relaxed inlier list
// is all that is left of it (the shuffled list goes to an empty LeastSquares, so only the draws are made: keep = 0).  Nothing reads that
// stream's values on this path, so the only observable effect of a run is the caller's lo_count; the draws are kept so that the stream stands
// where RansacLib's stands (a later estimator with a real LeastSquares would read it from there).
template <bool RAYS_LDS>
__device__ void l5_local_optimization(const double* model, const FpRays<RAYS_LDS>& rays, int n, const Lo5Opts& o, unsigned* mtR, int& posR, Lo5Shared* S) {
    if (6 > n) return;                                                                 // non_minimal_sample_size() > num_data
    const int ni = l5_count_inliers(model, rays, n, o.sq_thresh * o.thresh_mult, &S->cnt);
    if (ni < 5) return;
    block_shuffle_resize(nullptr, ni, 0, mtR, posR, o.fast_shuffle != 0, nullptr, &S->flag);
}

// what lomsac_trace.h asks of an estimator, over SteweniusEstimator
template <bool RAYS_LDS>
struct FivePointTraceEst {
    static constexpr int K = 5;
    static constexpr bool LO_CHANGES_MODEL = false;
    using Shared = Lo5Shared;
    FpRays<RAYS_LDS> rays; const double* pu; const double* pv; int n; Lo5Opts o; unsigned* mtR; int posR; Lo5Shared* S;

    // MinimalSolver + GetBestEstimatedModelId (ransac.h:184-195, 277-293)
    __device__ __forceinline__ int solve_and_score(const int* sample, double* myE, double* myScore) const {
        double u5[15], v5[15];
        for (int i = 0; i < 5; i++) {
            const int q = sample[i];
            for (int k = 0; k < 3; k++) { u5[3 * i + k] = pu[3 * q + k]; v5[3 * i + k] = pv[3 * q + k]; }
        }
        double Es[90];
        const int myNm = fp_minimal_solver(u5, v5, Es);
        // ScoreModel of the candidates, five per sweep over the rays: a ray is read once per sweep, the five chains are independent
        for (int m0 = 0; m0 < myNm; m0 += 5) {
            double Em[5][9], sc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int m = 0; m < 5; m++)
#pragma unroll
                for (int k = 0; k < 9; k++) Em[m][k] = (m0 + m < myNm) ? Es[9 * (m0 + m) + k] : 0.0;
            for (int i = 0; i < n; i++) {
                double a, b, v0, v1, v2; rays.get(i, &a, &b, &v0, &v1, &v2);
#pragma unroll
                for (int m = 0; m < 5; m++) sc[m] += fmin(fp_residual_n(Em[m], a, b, v0, v1, v2), o.sq_thresh);
            }
#pragma unroll
            for (int m = 0; m < 5; m++) if (m0 + m < myNm && sc[m] < *myScore) { *myScore = sc[m]; for (int k = 0; k < 9; k++) myE[k] = Em[m][k]; }
        }
        return myNm;
    }
    __device__ __forceinline__ void local_optimization(double* model, double*) { l5_local_optimization(model, rays, n, o, mtR, posR, S); }
    __device__ __forceinline__ int count_inliers(const double* model) { return l5_count_inliers(model, rays, n, o.sq_thresh, &S->cnt); }
};

template <bool RAYS_LDS>
__global__ void __launch_bounds__(L5_T, 2)
k_lomsac5_trace(const int* __restrict__ pair_ptr, const double* __restrict__ gu, const double* __restrict__ gv, Lo5Opts o,
                const unsigned* __restrict__ mt_seeded, double* __restrict__ outE, double* __restrict__ outScore, double* __restrict__ outR,
                double* __restrict__ outT, unsigned char* __restrict__ inlier_mask, int* __restrict__ num_inliers,
                unsigned* __restrict__ stats /* [pairs*2] iterations, LO runs; or null */) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ Lo5Shared S;
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int r0 = pair_ptr[pair], n = pair_ptr[pair + 1] - r0;
    const double MAXD = LO_MAXD;
    // dynamic LDS: [u0/u2 u1/u2 per ray | v per ray] (RAYS_LDS) then [mtS | mtR | fifo]
    double* sn = lds; double* sv = lds + (size_t)2 * n;
    unsigned* mtS = RAYS_LDS ? reinterpret_cast<unsigned*>(lds + (size_t)L5_RAY_DOUBLES * n) : reinterpret_cast<unsigned*>(lds);
    unsigned* mtR = mtS + 624; int* fifo = reinterpret_cast<int*>(mtR + 624);
    const double* pu = gu + (size_t)3 * r0; const double* pv = gv + (size_t)3 * r0;
    if (RAYS_LDS) {
        for (int i = tid; i < n; i += L5_T) { const double u2 = pu[3 * i + 2]; sn[2 * i] = pu[3 * i] / u2; sn[2 * i + 1] = pu[3 * i + 1] / u2; }
        for (int i = tid; i < 3 * n; i += L5_T) sv[i] = pv[i];
    }
    FpRays<RAYS_LDS> rays; rays.gu = pu; rays.gv = pv; rays.sn = sn; rays.sv = sv;
    for (int i = tid; i < 624; i += L5_T) { const unsigned w = mt_seeded[i]; mtS[i] = w; mtR[i] = w; }
    __syncthreads();

    double best_model[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double best_score = MAXD; unsigned it = 0, lo_count = 0;
    FivePointTraceEst<RAYS_LDS> est;
    est.rays = rays; est.pu = pu; est.pv = pv; est.n = n; est.o = o; est.mtR = mtR; est.posR = 624; est.S = &S;
    lomsac_trace(est, S, n, o, mtS, fifo, best_model, best_score, it, lo_count);
    // ---- estimate_pairwise_five_point's tail: inlier flags of E (spherical_sfm_tools.cpp:512-520), acceptance and PoseFromEssentialMatrix (:535-561)
    const bool have = (n >= 5) && best_score < MAXD;
    int mine = 0;
    for (int i = tid; i < n; i += L5_T) {
        const bool in = have && rays.residual(best_model, i) < o.sq_thresh;
        inlier_mask[r0 + i] = in ? 1 : 0; mine += in ? 1 : 0;
    }
    if (tid == 0) S.cnt = 0;
    __syncthreads();
    if (mine) atomicAdd(&S.cnt, mine);
    __syncthreads();
    const int nin = S.cnt;
    __syncthreads();
    double Rm[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tm[3] = {0, 0, 0};
    if (have && nin > o.min_num_inliers) { int votes[4]; fp_pose_block<RAYS_LDS>(best_model, rays, n, nullptr, inlier_mask + r0, S.votes, Rm, tm, votes); }
    if (tid == 0) {
        num_inliers[pair] = nin;
        for (int k = 0; k < 9; k++) { outR[9 * (size_t)pair + k] = Rm[k]; outE[9 * (size_t)pair + k] = best_model[k]; }
        for (int k = 0; k < 3; k++) outT[3 * (size_t)pair + k] = tm[k];
        outScore[pair] = best_score;
        if (stats) { stats[2 * (size_t)pair] = it; stats[2 * (size_t)pair + 1] = lo_count; }
    }
}

// ---- probes: each calls the device function the trace kernel calls ---------------------------------------------------------------
// fp_minimal_solver, lane per sample; Es [S*90] row-major, zero beyond the count
__global__ void k_fp_solver_probe(int S, const int* __restrict__ sample, const double* __restrict__ u, const double* __restrict__ v,
                                  double* __restrict__ Es, int* __restrict__ counts) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    double u5[15], v5[15], E[90];
    for (int i = 0; i < 5; i++) for (int k = 0; k < 3; k++) { u5[3 * i + k] = u[3 * (size_t)sample[5 * s + i] + k]; v5[3 * i + k] = v[3 * (size_t)sample[5 * s + i] + k]; }
    const int c = fp_minimal_solver(u5, v5, E);
    counts[s] = c;
    for (int k = 0; k < 90; k++) Es[90 * (size_t)s + k] = (k < 9 * c) ? E[k] : 0.0;
}
// fp_residual of T models on n rays: err[t*n + i]
__global__ void k_fp_residual_probe(int T, int n, const double* __restrict__ Es, const double* __restrict__ u, const double* __restrict__ v, double* __restrict__ err) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (i >= n || t >= T) return;
    double E[9]; for (int k = 0; k < 9; k++) E[k] = Es[9 * (size_t)t + k];
    FpRays<false> rays; rays.gu = u; rays.gv = v; rays.sn = nullptr; rays.sv = nullptr;
    err[(size_t)t * n + i] = rays.residual(E, i);
}
// fp_pose_block, workgroup per task: out [tasks*12] = R (row-major) | t, votes [tasks*4]
__global__ void __launch_bounds__(L5_T)
k_fp_pose_probe(const double* __restrict__ u, const double* __restrict__ v, const int* __restrict__ task_ptr, const int* __restrict__ lists,
                const double* __restrict__ Ein, double* __restrict__ out, int* __restrict__ votes_out) {
    __shared__ int s_votes[4];
    const int t = blockIdx.x, l0 = task_ptr[t], cnt = task_ptr[t + 1] - l0;
    double E[9]; for (int k = 0; k < 9; k++) E[k] = Ein[9 * (size_t)t + k];
    FpRays<false> rays; rays.gu = u; rays.gv = v; rays.sn = nullptr; rays.sv = nullptr;
    double R[9], tt[3]; int votes[4];
    fp_pose_block<false>(E, rays, cnt, lists + l0, nullptr, s_votes, R, tt, votes);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 9; k++) out[12 * (size_t)t + k] = R[k];
        for (int k = 0; k < 3; k++) out[12 * (size_t)t + 9 + k] = tt[k];
        for (int k = 0; k < 4; k++) votes_out[4 * (size_t)t + k] = votes[k];
    }
}

// One slab of pairs through the trace kernel; device buffers are the caller's.  Used by ransac.hip's batch driver.
static bool l5_force_global() { const char* e = getenv("SSFM_RANSAC5_FORCE_GLOBAL"); return e && atoi(e) != 0; }       // read at call time (tests)
int lomsac5_launch(ssfm_ctx* ctx, hipStream_t st, int num_pairs, int max_n, const int* d_pair_ptr, const double* d_u, const double* d_v,
                   const ssfm_ransac_options& O, double sq_thresh, const unsigned* d_mt_seeded, double* d_E, double* d_score, double* d_R, double* d_t,
                   unsigned char* d_mask, int* d_nin, unsigned* d_stats) {
    Lo5Opts o;
    lo_trace_opts(O, sq_thresh, &o);
    const bool in_lds = max_n <= l5_max_lds_rays() && !l5_force_global();
    const size_t lds = in_lds ? (size_t)L5_RAY_DOUBLES * max_n * sizeof(double) + L5_LDS_FIXED : L5_LDS_FIXED;
    return lo_trace_launch(ctx, st, in_lds ? k_lomsac5_trace<true> : k_lomsac5_trace<false>, num_pairs, lds,
                           d_pair_ptr, d_u, d_v, o, d_mt_seeded, d_E, d_score, d_R, d_t, d_mask, d_nin, d_stats);
}
}  // namespace ssfm
using namespace ssfm;

// ---- C ABI: probes -----------------------------------------------------------------------------------------------------------
extern "C" int32_t ssfm_fivepoint_max_lds_rays(void) { return l5_max_lds_rays(); }

extern "C" int ssfm_fivepoint_solver_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t S, const int32_t* samples, double* Es, int32_t* counts) {
    if (!ctx || n <= 0 || !u || !v || S <= 0 || !samples || !Es || !counts) return fail(ctx, SSFM_ERR_INVALID, "ssfm_fivepoint_solver_probe: bad arguments");
    for (int64_t i = 0; i < (int64_t)5 * S; i++) if (samples[i] < 0 || samples[i] >= n) return fail(ctx, SSFM_ERR_INVALID, "ssfm_fivepoint_solver_probe: index out of range");
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<double> hu(u, u + (size_t)3 * n), hv(v, v + (size_t)3 * n), hE((size_t)90 * S); std::vector<int> hs(samples, samples + (size_t)5 * S);
    {
        DevBuf<double> du, dv, dE; DevBuf<int> ds, dc;
        DevBufScope scope(du, dv, dE, ds, dc);
        SSFM_HIP_CHECK(ctx, upload(du, hu, st)); SSFM_HIP_CHECK(ctx, upload(dv, hv, st)); SSFM_HIP_CHECK(ctx, upload(ds, hs, st));
        SSFM_HIP_CHECK(ctx, dE.alloc((size_t)90 * S)); SSFM_HIP_CHECK(ctx, dc.alloc(S));
        hipLaunchKernelGGL(k_fp_solver_probe, dim3((S + 63) / 64), dim3(64), 0, st, S, ds.p, du.p, dv.p, dE.p, dc.p);
        SSFM_HIP_CHECK(ctx, hipGetLastError());
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(hE.data(), dE.p, hE.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(counts, dc.p, S * sizeof(int), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    for (int s = 0; s < S; s++) for (int m = 0; m < 10; m++) rm_to_cm(&hE[90 * (size_t)s + 9 * m], Es + 90 * (size_t)s + 9 * m);
    return SSFM_OK;
}

extern "C" int ssfm_fivepoint_residual_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t T, const double* Es, double* errors) {
    if (!ctx || n <= 0 || !u || !v || T <= 0 || !Es || !errors) return fail(ctx, SSFM_ERR_INVALID, "ssfm_fivepoint_residual_probe: bad arguments");
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<double> hu(u, u + (size_t)3 * n), hv(v, v + (size_t)3 * n), hE((size_t)9 * T);
    for (int t = 0; t < T; t++) cm_to_rm(Es + 9 * (size_t)t, &hE[9 * (size_t)t]);
    DevBuf<double> du, dv, dE, derr;
    DevBufScope scope(du, dv, dE, derr);
    SSFM_HIP_CHECK(ctx, upload(du, hu, st)); SSFM_HIP_CHECK(ctx, upload(dv, hv, st)); SSFM_HIP_CHECK(ctx, upload(dE, hE, st)); SSFM_HIP_CHECK(ctx, derr.alloc((size_t)T * n));
    hipLaunchKernelGGL(k_fp_residual_probe, dim3((n + 255) / 256, T), dim3(256), 0, st, T, n, dE.p, du.p, dv.p, derr.p);
    SSFM_HIP_CHECK(ctx, hipGetLastError());
    SSFM_HIP_CHECK(ctx, hipMemcpyAsync(errors, derr.p, (size_t)T * n * sizeof(double), hipMemcpyDeviceToHost, st));
    SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return SSFM_OK;
}

extern "C" int ssfm_fivepoint_pose_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t tasks, const int32_t* task_ptr, const int32_t* lists,
                                         const double* E, double* R_out, double* t_out, int32_t* votes) {
    if (!ctx || n <= 0 || !u || !v || tasks <= 0 || !task_ptr || !lists || !E) return fail(ctx, SSFM_ERR_INVALID, "ssfm_fivepoint_pose_probe: bad arguments");
    for (int t = 0; t < tasks; t++) if (task_ptr[t + 1] < task_ptr[t] || task_ptr[t] < 0) return fail(ctx, SSFM_ERR_INVALID, "ssfm_fivepoint_pose_probe: task_ptr must ascend");
    const int nl = task_ptr[tasks];
    for (int i = 0; i < nl; i++) if (lists[i] < 0 || lists[i] >= n) return fail(ctx, SSFM_ERR_INVALID, "ssfm_fivepoint_pose_probe: index out of range");
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<double> hu(u, u + (size_t)3 * n), hv(v, v + (size_t)3 * n), hE((size_t)9 * tasks), hout((size_t)12 * tasks);
    for (int t = 0; t < tasks; t++) cm_to_rm(E + 9 * (size_t)t, &hE[9 * (size_t)t]);
    std::vector<int> hp(task_ptr, task_ptr + tasks + 1), hl(lists, lists + nl), hvotes((size_t)4 * tasks); if (hl.empty()) hl.push_back(0);
    {
        DevBuf<double> du, dv, dE, dout; DevBuf<int> dp, dl, dvt;
        DevBufScope scope(du, dv, dE, dout, dp, dl, dvt);
        SSFM_HIP_CHECK(ctx, upload(du, hu, st)); SSFM_HIP_CHECK(ctx, upload(dv, hv, st)); SSFM_HIP_CHECK(ctx, upload(dE, hE, st));
        SSFM_HIP_CHECK(ctx, upload(dp, hp, st)); SSFM_HIP_CHECK(ctx, upload(dl, hl, st));
        SSFM_HIP_CHECK(ctx, dout.alloc((size_t)12 * tasks)); SSFM_HIP_CHECK(ctx, dvt.alloc((size_t)4 * tasks));
        hipLaunchKernelGGL(k_fp_pose_probe, dim3(tasks), dim3(L5_T), 0, st, du.p, dv.p, dp.p, dl.p, dE.p, dout.p, dvt.p);
        SSFM_HIP_CHECK(ctx, hipGetLastError());
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(hout.data(), dout.p, hout.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(hvotes.data(), dvt.p, hvotes.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    for (int t = 0; t < tasks; t++) {
        if (R_out) rm_to_cm(&hout[12 * (size_t)t], R_out + 9 * (size_t)t);
        if (t_out) for (int k = 0; k < 3; k++) t_out[3 * (size_t)t + k] = hout[12 * (size_t)t + 9 + k];
        if (votes) for (int k = 0; k < 4; k++) votes[4 * (size_t)t + k] = hvotes[4 * (size_t)t + k];
    }
    return SSFM_OK;
}
