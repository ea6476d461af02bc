// spherical_sfm_amd -- what match.hip, ransac.hip and pairwise_front.hip share so that ssfm_pairwise_from_features and ssfm_pairwise5_from_features can run
// the existing matching and LO-MSAC kernels with the match lists staying on the device.
#pragma once
#include <functional>
#include "ssfm_ctx.h"

namespace ssfm {

// exclusive prefix sum of one int per thread over a 256-thread workgroup (a wave scan + one LDS pass); *total = the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int* total) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    __syncthreads();                                               // (wsum of the previous call has been read)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, all = 0;
    for (int w = 0; w < 4; w++) { if (w < wave) base += wsum[w]; all += wsum[w]; }
    *total = all;
    return base + inc - v;
}

// ---- match.hip ------------------------------------------------------------------------------------------------------------------
// The argument checks of ssfm_match_pairs on the feature tables, the pair list and the options (`who` prefixes the message); *O = the options in force.
int match_check_args(ssfm_ctx* ctx, const char* who, int32_t num_frames, const int32_t* feat_ptr, const float* descs, int32_t num_pairs, const int32_t* pair_frame0,
                     const int32_t* pair_frame1, const ssfm_match_options* opt, ssfm_match_options* O);
// One slab of pairs [p0, p0 + np) has been matched: hptr [np + 1] is its exclusive count scan on the host, d_idx0 / d_idx1 its compacted lists on the
// device (valid until the sink returns; the stream is idle).  A non-zero return ends the run with that code.
typedef std::function<int(int p0, int np, const int* hptr, const int* d_idx0, const int* d_idx1)> MatchSlabSink;
// The slab loop of ssfm_match_pairs (arguments already checked): upload, |t|^2, distances, compaction; only the count scan comes back per slab.
// Sets ctx->match_kernel_ms.
int match_slabs(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, int32_t num_pairs, const int32_t* pair_frame0,
                const int32_t* pair_frame1, const ssfm_match_options& O, const MatchSlabSink& sink);

// ---- ransac.hip -----------------------------------------------------------------------------------------------------------------
// ransac_batch_impl on match lists that are already on the device.  The slab plan, the kernels and their launch parameters are those of
// ssfm_ransac_batch_indexed -- with five = true those of ssfm_ransac5_batch_indexed (k_lomsac5_trace; the options go through ransac5_options and `who` names
// the entry point in the messages); the hooks replace the host staging of the lists (stage / gather) and the copy of the inlier mask (lists / collect).
// `slot` is the double-buffer slot (0 / 1) of the slab, p0 / np its pairs; d_ptr is the slab-local CSR of its correspondences.  d_R / d_E [9 np] are
// row-major, d_t [3 np]; d_E and d_t are null in spherical mode.
struct RansacDeviceLists {
    virtual int prepare(int nslot, int cap_pairs, size_t cap_rays) = 0;                        // per-slot buffers
    virtual int stage(hipStream_t up, int slot, int p0, int np) = 0;                           // the slab's per-pair source table, on the upload stream
    virtual int gather(hipStream_t st, int slot, int np, const int* d_ptr, double* d_u, double* d_v) = 0;
    virtual int lists(hipStream_t st, int slot, int np, const int* d_ptr, const unsigned char* d_mask, const int* d_nin, const double* d_R, const double* d_E,
                      const double* d_t) = 0;                                                  // after the RANSAC kernels
    virtual int collect(hipStream_t cp, int slot, int p0, int np) = 0;                         // the slab has finished: copy back what was accepted
    virtual ~RansacDeviceLists() {}
};
int ransac_on_device_lists(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, int32_t num_pairs, const int32_t* pair_frame0, const int32_t* pair_frame1,
                           const int32_t* pair_ptr, double sq_thresh, const ssfm_ransac_options& O, RansacDeviceLists* hooks, int32_t* num_inliers, uint32_t* stats,
                           bool five = false, const char* who = nullptr);

}  // namespace ssfm
