// spherical_sfm_amd -- the control flow of ransac_lib::LocallyOptimizedMSAC::EstimateModel with the reference's own sample trace, once,
// for every estimator that runs it on the device (k_lomsac_trace in lomsac.hip, k_lomsac5_trace in fivepoint.hip).
//
//   LocallyOptimizedMSAC<...>::EstimateModel                                       include/RansacLib/ransac.h:128-275
//   UniformSampling (std::mt19937 seeded with random_seed_, DrawSample / ShuffleSample)   include/RansacLib/sampling.h:46-135
//   utils::NumRequiredIterations                                                     include/RansacLib/utils.h:110-140
//
// One workgroup of LO_T threads per image pair.  A chunk of iterations is evaluated at once, one lane per iteration: the sampler's stream
// does not depend on the models, so its draws run ahead (phase A); every lane solves and scores its own minimal sample (phase B, the
// estimator's); the control flow then walks the chunk in order (phase C), and the rare events of the walk (a new best minimal model, a local
// optimisation, the refresh of the iteration bound) are workgroup-cooperative calls into the estimator.
//
// What an estimator policy `Est` supplies:
//   static constexpr int K                       size of a minimal sample
//   static constexpr bool LO_CHANGES_MODEL       false: LocalOptimization returns its model and score untouched, so best_model and
//                                                best_minimal_model of EstimateModel are always the same matrix and only one is kept
//   typename Shared                              the kernel's static LDS, with double score[LO_T], E[9]; int sample[K * LO_T], nm[LO_T]
//   int solve_and_score(const int* sample, double* E, double* score)         one lane: MinimalSolver + GetBestEstimatedModelId
//                                                (ransac.h:184-195, 277-293); returns the number of models, E / score only where one wins
//   void local_optimization(double* model, double* score)                    the workgroup: LocalOptimization (ransac.h:341-407)
//   int count_inliers(const double* model)                                   the workgroup: GetInliers(model).size() (ransac.h:311-336)
#pragma once
#include "ransac_device.h"

namespace ssfm {

constexpr int LO_T = 128;          // threads per pair: RansacLib never stops before min_num_iterations_ = 100 and usually stops there, so the first chunk is those 100 iterations
constexpr double LO_MAXD = 1.79769313486231570815e308;      // std::numeric_limits<double>::max(): "no model yet"

constexpr int lo_fifo_len(int K) { return K * LO_T + 64; }  // pre-drawn sampler indices (K per iteration + spare for repeated indices)
constexpr size_t lo_lds_fixed(int K) { return (size_t)(2 * 624 + lo_fifo_len(K)) * 4; }      // dynamic LDS behind the rays: [mtS | mtR | fifo]

// DrawBetterThanShuffle (sampling.h:66-75): a sample of K from n is drawn index by index when n / (n - K) < e, else (0..n-1) is shuffled
constexpr bool lo_draw_better_than_shuffle(int n, int K) { return ((double)n / (double)(n - K)) < 2.71828182845904523536; }
constexpr int lo_max_shuffle_n(int K) { int n = K; while (!lo_draw_better_than_shuffle(n + 1, K)) n++; return n; }     // the largest n that ShuffleSample sees
static_assert(lo_max_shuffle_n(3) == 4 && lo_max_shuffle_n(5) == 7, "ShuffleSample's scratch array is sized by this");

// the RansacOptions / LORansacOptions fields the control flow itself reads (an estimator's own options derive from it)
struct LoTraceOpts {
    double sq_thresh, thresh_mult, success_prob;
    unsigned min_it, max_it, lo_start;
    int min_num_inliers, fast_shuffle;
};
inline void lo_trace_opts(const ssfm_ransac_options& O, double sq_thresh, LoTraceOpts* o) {
    o->sq_thresh = sq_thresh; o->thresh_mult = O.threshold_multiplier; o->success_prob = O.success_probability;
    o->min_it = O.min_num_iterations; o->max_it = O.max_num_iterations; o->lo_start = O.lo_starting_iterations;
    o->min_num_inliers = O.min_num_inliers; o->fast_shuffle = O.fast_shuffle;
}

// one workgroup per pair, `lds` bytes of dynamic LDS (above 48 KiB the kernel has to be told first)
template <typename... P, typename... A>
int lo_trace_launch(ssfm_ctx* ctx, hipStream_t st, void (*kernel)(P...), int num_pairs, size_t lds, A... args) {
    if (lds > 48 * 1024) SSFM_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3(num_pairs), dim3(LO_T), lds, st, args...);
    SSFM_HIP_CHECK(ctx, hipGetLastError());
    return SSFM_OK;
}

__device__ __forceinline__ void lo_update(double sc, const double* m, double* best_sc, double* best) { if (sc < *best_sc) { *best_sc = sc; for (int k = 0; k < 9; k++) best[k] = m[k]; } }

// EstimateModel for a pair of n correspondences, every thread of the workgroup with the same arguments.  mtS: the sampler's generator state
// (624 words, seeded) with fifo (lo_fifo_len(K) ints) behind it, both in LDS.  best_model / best_score / it / lo_count come in as
// EstimateModel initialises them (zero, LO_MAXD, 0, 0) and go out as it returns them, before the final least squares.
template <typename Est>
__device__ __forceinline__ void lomsac_trace(Est& est, typename Est::Shared& S, int n, const LoTraceOpts& o, unsigned* mtS, int* fifo,
                                             double* best_model, double& best_score, unsigned& it, unsigned& lo_count) {
    constexpr int K = Est::K, FIFO = lo_fifo_len(K);
    const int tid = threadIdx.x;
    if (n < K) return;                                                                  // ransac.h:137-141
    int posS = 624, fifo_head = 0, fifo_cnt = 0;
    const bool draw = lo_draw_better_than_shuffle(n, K);
    unsigned max_it = max(o.max_it, o.min_it);
    // best_minimal_model of EstimateModel and its score.  Where LocalOptimization can move best_model away from it (LO_CHANGES_MODEL) it is a matrix of
    // its own, own_min.  Where it cannot, the two are always equal and best_min / best_min_score ALIAS best_model / best_score: phase C then writes
    // best_model through best_min, the lo_update calls (which would copy a matrix onto itself) are compiled out, and own_min is a dead array of one.
    [[maybe_unused]] double own_min[Est::LO_CHANGES_MODEL ? 9 : 1] = {0}; [[maybe_unused]] double own_min_score = LO_MAXD;
    double* best_min; double* best_min_score;
    if constexpr (Est::LO_CHANGES_MODEL) { best_min = own_min; best_min_score = &own_min_score; } else { best_min = best_model; best_min_score = &best_score; }
    auto refresh = [&]() {
        // GetInliers(best_model) -> best_num_inliers, inlier_ratio -> max_num_iterations  (ransac.h:169-176, 229-236)
        const int best_num_inliers = est.count_inliers(best_model);
        max_it = num_required_iterations((double)best_num_inliers / (double)n, 1.0 - o.success_prob, K, o.min_it, o.max_it);
    };
    bool done = false;
    while (!done && it < max_it) {
        // ---- chunk of iterations [it, it + cnt)
        unsigned cnt = min((unsigned)LO_T, max_it - it);
        if (it < o.min_it) cnt = min(cnt, o.min_it - it);                               // never fewer than min_num_iterations_ are run
        // phase A: the minimal samples of the chunk, in order (the sampler's stream is independent of everything else)
        if (draw) {
            for (unsigned c = 0; c < cnt; c++) {
                int smp[K];
                for (int i = 0; i < K; i++) {
                    bool found = true;
                    while (found) {
                        if (fifo_head >= fifo_cnt) {
                            // refill: temper the next words of the stream in parallel; -1 marks a Lemire rejection (the draw is repeated)
                            __syncthreads();                       // every thread has read the last entry before it is overwritten
                            fifo_head = 0; fifo_cnt = 0;
                            while (fifo_cnt < FIFO) {
                                if (posS >= 624) { mt_twist(mtS); posS = 0; }
                                const int seg = min(FIFO - fifo_cnt, 624 - posS);
                                for (int j = tid; j < seg; j += LO_T) { unsigned r; const bool ok = lemire_accept(mt_temper(mtS[posS + j]), (unsigned)n, &r); fifo[fifo_cnt + j] = ok ? (int)r : -1; }
                                posS += seg; fifo_cnt += seg;
                            }
                            __syncthreads();
                        }
                        const int d = fifo[fifo_head++];
                        if (d < 0) continue;
                        smp[i] = d; found = false;
                        for (int j = 0; j < i; j++) if (smp[j] == d) { found = true; break; }
                    }
                }
                if (tid == 0) for (int i = 0; i < K; i++) S.sample[K * c + i] = smp[i];
            }
        } else {
            // ShuffleSample (sampling.h:104-124): n = K takes (0..K-1) without a draw, a larger n shuffles (0..n-1) and keeps the first K
            for (unsigned c = 0; c < cnt; c++) {
                int p[lo_max_shuffle_n(K)];
                for (int i = 0; i < lo_max_shuffle_n(K); i++) p[i] = i;
                if (n != K) for (int i = 0; i < n - 1; i++) { const int idx = mt_uniform_int(mtS, posS, i, n - 1); const int t = p[i]; p[i] = p[idx]; p[idx] = t; }
                if (tid == 0) for (int i = 0; i < K; i++) S.sample[K * c + i] = p[i];
            }
        }
        __syncthreads();
        // phase B: one lane per iteration
        double myE[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; double myScore = LO_MAXD; int myNm = 0;
        if ((unsigned)tid < cnt) myNm = est.solve_and_score(S.sample + K * tid, myE, &myScore);
        S.score[tid] = myScore; S.nm[tid] = myNm;
        __syncthreads();
        // phase C: the control flow of EstimateModel over the chunk, in order
        for (unsigned c = 0; c < cnt; c++) {
            if (it >= max_it) { done = true; break; }
            if (it == o.lo_start && *best_min_score < LO_MAXD) {                        // ransac.h:160-177
                ++lo_count;
                est.local_optimization(best_model, &best_score);
                refresh();
            }
            const int nm = S.nm[c]; const double bl = S.score[c];
            if (nm > 0 && (bl < *best_min_score || it == o.lo_start)) {                 // ransac.h:197-237
                const bool best_min_model = bl < *best_min_score;
                __syncthreads();
                if (best_min_model) {
                    if ((unsigned)tid == c) for (int k = 0; k < 9; k++) S.E[k] = myE[k];
                    __syncthreads();
                    *best_min_score = bl; for (int k = 0; k < 9; k++) best_min[k] = S.E[k];
                    if constexpr (Est::LO_CHANGES_MODEL) lo_update(*best_min_score, best_min, &best_score, best_model);
                }
                __syncthreads();
                const bool run_lo = (it >= o.lo_start && *best_min_score < LO_MAXD);
                if (best_min_model || run_lo) {
                    if (run_lo) {
                        ++lo_count;
                        double sc = *best_min_score;
                        est.local_optimization(best_min, &sc);
                        if constexpr (Est::LO_CHANGES_MODEL) lo_update(sc, best_min, &best_score, best_model);
                    }
                    refresh();
                }
            }
            ++it;
        }
        __syncthreads();
    }
    if (it <= o.lo_start && best_score < LO_MAXD) {                                     // ransac.h:241-251
        ++lo_count;
        est.local_optimization(best_model, &best_score);
        // RansacLib runs GetInliers here; nothing reads the count any more.  The call is kept only so that the spherical kernel passes the same barriers
        // and does the same work as before the control flow was shared (the five-point kernel never made it); it can go, with a new timing
        if constexpr (Est::LO_CHANGES_MODEL) (void)est.count_inliers(best_model);
    }
}

}  // namespace ssfm
