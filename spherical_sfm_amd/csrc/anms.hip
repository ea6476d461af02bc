// spherical_sfm_amd -- adaptive non-maximal suppression of keypoints, batched over frames: adaptiveNonMaximalSuppresion of the reference
// (examples/spherical_sfm_tools.cpp:76-123), the thinning step of DetectorTracker::detect (:179-208).  The contract is in include/ssfm.h.
//
// The reference sorts by response and walks, for every keypoint, the prefix of stronger ones.  Here nothing is sorted.  With the total order
//   precedes(j, i) = response_j > response_i || (response_j == response_i && j < i)
// the reference's loop is   radius_i = sqrt(min over {j : response_j > thr_i && precedes(j, i)} of d2(i, j)),   and   rank_i = #{j : precedes(j, i)}
// is keypoint i's position in the sorted list.  d2 = (double)dx * dx + (double)dy * dy with dx, dy float differences: both products are exact in double, so the
// sum is one rounding whether or not the compiler fuses it, and sqrt, monotone and correctly rounded, is taken once, of the minimum.
//
//   k_anms_radius   one workgroup per work item (frame, 256 keypoints i, chunk of keypoints j) of anms_host.h's plan.  A lane owns one i in registers; the j go
//                   through LDS in tiles of 1024 (x, y, response, 16 B each), every lane reads the same j (a broadcast read).  Per j: the predicate, two float
//                   subtractions, the double sum of squares, a running minimum, the rank count.  The index only decides among the workgroup's own 256 keypoints:
//                   the j before them and the j after them run with one comparison for `precedes`.  A frame whose j range is cut combines the chunks with a 64-bit
//                   unsigned atomicMin on the bit pattern of d2 (non-negative doubles order like their patterns) and an integer atomicAdd on the rank: both are
//                   order-independent, the result is the same bits however the chunks arrive.  An uncut frame stores.
//   k_anms_select   one workgroup per frame.  radius = sqrt(d2) (DBL_MAX where no j qualified); the (num_to_keep + 1)-th largest radius by radix selection on the
//                   64-bit patterns, eight passes of eight bits; radius >= decision is flagged; the kept indices go to slot rank_i; a scan over the slots compacts
//                   them, so the list comes out in sorted order.  The comparison is made on the square-rooted radii, as the reference makes it: two d2 can share
//                   one square root.
#include <algorithm>
#include <cfloat>
#include <cstring>
#include "dev_buf.h"
#include "anms_host.h"

namespace ssfm {

constexpr unsigned long long kAnmsInfBits = 0x7FF0000000000000ull;       // +infinity: "no j yet"
constexpr int kAnmsSelectThreads = 1024;

struct AnmsFrameDev { int32_t kp0, n, keep, reserved; };

__global__ void __launch_bounds__(256)
k_anms_init(int total, unsigned long long* __restrict__ d2bits, int* __restrict__ rank) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < total) { d2bits[g] = kAnmsInfBits; rank[g] = 0; }
}

// Which side of a lane's own keypoint a run of j lies on decides how the tie of equal responses falls: every j of the run before every i of the workgroup
// (precedes = response_j >= response_i), every j after every i (response_j > response_i), or the run that holds the workgroup's own i (the index decides).
enum { kAnmsBefore = 0, kAnmsOwn = 1, kAnmsAfter = 2 };

// The keypoints j_lo .. j_hi of the frame at kp0 against the lane's keypoint i, tile by tile through LDS.  All lanes of the workgroup call it with the same range.
template <int SIDE>
__device__ __forceinline__ void anms_run(float4* tile, const float2* __restrict__ xy, const float* __restrict__ resp, int kp0, int j_lo, int j_hi, int i, float2 pi,
                                         float ri, float thr, double& m, int& cnt) {
    const int tid = threadIdx.x;
    for (int j0 = j_lo; j0 < j_hi; j0 += kAnmsTile) {
        const int len = min(kAnmsTile, j_hi - j0);
        for (int t = tid; t < len; t += kAnmsBlock) {
            const float2 p = xy[(size_t)kp0 + (size_t)(j0 + t)];
            tile[t] = make_float4(p.x, p.y, resp[(size_t)kp0 + (size_t)(j0 + t)], 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < len; t++) {
            const float4 q = tile[t];
            // `|` and `&` on purpose: with `||` / `&&` the compiler branches on the execution mask and waits for every LDS read on its own
            const bool pre = SIDE == kAnmsBefore ? q.z >= ri : SIDE == kAnmsAfter ? q.z > ri : ((q.z > ri) | ((q.z == ri) & (j0 + t < i)));
            cnt += pre ? 1 : 0;
            const float dx = pi.x - q.x, dy = pi.y - q.y;
            const double d = (double)dx * (double)dx + (double)dy * (double)dy;
            m = (pre & (q.z > thr) & (d < m)) ? d : m;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kAnmsBlock)
k_anms_radius(const AnmsItem* __restrict__ items, const float2* __restrict__ xy, const float* __restrict__ resp, unsigned long long* __restrict__ d2bits,
              int* __restrict__ rank) {
    __shared__ float4 tile[kAnmsTile];
    const AnmsItem it = items[blockIdx.x];
    const int tid = threadIdx.x, i = it.i0 + tid;
    const bool valid = i < it.n;
    const size_t gi = (size_t)it.kp0 + (size_t)(valid ? i : it.n - 1);          // a lane past the end works on the last keypoint and stores nothing
    const float2 pi = xy[gi];
    const float ri = resp[gi], thr = ri * 1.11f;
    double m = __longlong_as_double((long long)kAnmsInfBits);
    int cnt = 0;
    // the item's j range in three runs: before the workgroup's keypoints i0 .. i0 + 256, among them, after them (each may be empty)
    const int own_lo = min(max(it.i0, it.j_lo), it.j_hi), own_hi = max(min(it.i0 + kAnmsBlock, it.j_hi), own_lo);
    anms_run<kAnmsBefore>(tile, xy, resp, it.kp0, it.j_lo, own_lo, i, pi, ri, thr, m, cnt);
    anms_run<kAnmsOwn>(tile, xy, resp, it.kp0, own_lo, own_hi, i, pi, ri, thr, m, cnt);
    anms_run<kAnmsAfter>(tile, xy, resp, it.kp0, own_hi, it.j_hi, i, pi, ri, thr, m, cnt);
    if (!valid) return;
    const unsigned long long mb = (unsigned long long)__double_as_longlong(m);
    if (it.split) {
        if (mb != kAnmsInfBits) atomicMin(&d2bits[gi], mb);
        if (cnt) atomicAdd(&rank[gi], cnt);
    } else {
        d2bits[gi] = mb; rank[gi] = cnt;
    }
}

__global__ void __launch_bounds__(kAnmsSelectThreads)
k_anms_select(const AnmsFrameDev* __restrict__ frames, const unsigned long long* __restrict__ d2bits, const int* __restrict__ rank, double* __restrict__ radius,
              int* __restrict__ slot, int* __restrict__ keep_idx, int* __restrict__ count) {
    __shared__ int hist[256];
    __shared__ int wave_tot[kAnmsSelectThreads / 64];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_remaining;
    const AnmsFrameDev F = frames[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = F.n;
    const size_t base = (size_t)F.kp0;
    if (n < F.keep) {                                                            // returned unchanged
        for (int i = tid; i < n; i += kAnmsSelectThreads) { keep_idx[base + i] = i; radius[base + i] = DBL_MAX; }
        if (tid == 0) count[blockIdx.x] = n;
        return;
    }
    for (int i = tid; i < n; i += kAnmsSelectThreads) {
        const unsigned long long b = d2bits[base + i];
        radius[base + i] = b == kAnmsInfBits ? DBL_MAX : sqrt(__longlong_as_double((long long)b));
    }
    if (tid == 0) { s_prefix = 0ull; s_remaining = F.keep; }
    __syncthreads();
    unsigned long long decision = 0ull;                                          // n == num_to_keep: everything is kept
    if (F.keep < n) {
        // element `keep` (0-based) of the radii sorted descending: most significant byte first, walking each histogram from the top
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int b = tid; b < 256; b += kAnmsSelectThreads) hist[b] = 0;
            __syncthreads();
            const unsigned long long prefix = s_prefix;
            for (int i = tid; i < n; i += kAnmsSelectThreads) {
                const unsigned long long v = (unsigned long long)__double_as_longlong(radius[base + i]);
                if (shift == 56 || (v >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((v >> shift) & 255ull)], 1);
            }
            __syncthreads();
            if (wave == 0) {
                // lane l owns the bins 255 - 4 l .. 252 - 4 l; a wave prefix sum in descending bin order finds the lane whose bins hold the element
                const int rem = s_remaining, top = 255 - 4 * lane;
                const int h0 = hist[top], h1 = hist[top - 1], h2 = hist[top - 2], h3 = hist[top - 3];
                const int s = h0 + h1 + h2 + h3;
                int incl = s;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                int r = rem - (incl - s);
                if (r >= 0 && r < s) {                                           // exactly one lane: the counts above the prefix sum to more than rem
                    int bin = top;
                    if (r >= h0) { r -= h0; bin--; if (r >= h1) { r -= h1; bin--; if (r >= h2) { r -= h2; bin--; } } }
                    s_prefix = (prefix << 8) | (unsigned long long)bin;
                    s_remaining = r;
                }
            }
            __syncthreads();
        }
        decision = s_prefix;
    }
    const double dec = __longlong_as_double((long long)decision);
    for (int i = tid; i < n; i += kAnmsSelectThreads) {
        const int rk = rank[base + i];
        if ((unsigned)rk < (unsigned)n) slot[base + rk] = radius[base + i] >= dec ? i : -1;
    }
    __syncthreads();                                                             // the slots are this workgroup's own global writes
    int kept = 0;
    for (int p0 = 0; p0 < n; p0 += kAnmsSelectThreads) {
        const int p = p0 + tid;
        const int v = p < n ? slot[base + p] : -1;
        const unsigned long long mask = __ballot(v >= 0);
        if (lane == 0) wave_tot[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kAnmsSelectThreads / 64; w++) { const int t = wave_tot[w]; all += t; before += w < wave ? t : 0; }
        if (v >= 0) keep_idx[base + kept + before + __popcll(mask & ((1ull << lane) - 1ull))] = v;
        kept += all;
        __syncthreads();
    }
    if (tid == 0) count[blockIdx.x] = kept;
}

}  // namespace ssfm
using namespace ssfm;

#define ANMS_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipStreamSynchronize(st); release(); return fail(ctx, SSFM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)

extern "C" void ssfm_anms_default_options(ssfm_anms_options* o) {
    if (!o) return;
    o->force_j_chunks = 0; o->reserved = 0;
}

extern "C" int ssfm_anms_last_kernel_ms(ssfm_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SSFM_ERR_INVALID;
    *ms = ctx->anms_kernel_ms;
    return SSFM_OK;
}

extern "C" int ssfm_anms_batch_host(int32_t num_frames, const int32_t* kp_ptr, const float* xy, const float* response, const int32_t* num_to_keep,
                                    int32_t num_threads, int32_t* keep_ptr, int32_t* keep_idx, double* radius) {
    const char* who = "ssfm_anms_batch_host";
    if (const char* why = anms_check(num_frames, kp_ptr, xy, response, num_to_keep, nullptr, keep_ptr, keep_idx)) return fail(nullptr, SSFM_ERR_INVALID, std::string(who) + ": " + why);
    anms_batch_host(num_frames, kp_ptr, xy, response, num_to_keep, num_threads, keep_ptr, keep_idx, radius);
    return SSFM_OK;
}

extern "C" int ssfm_anms_batch(ssfm_ctx* ctx, int32_t num_frames, const int32_t* kp_ptr, const float* xy, const float* response, const int32_t* num_to_keep,
                               const ssfm_anms_options* opt, int32_t* keep_ptr, int32_t* keep_idx, double* radius) {
    const char* who = "ssfm_anms_batch";
    if (const char* why = anms_check(num_frames, kp_ptr, xy, response, num_to_keep, opt, keep_ptr, keep_idx)) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": " + why);
    if (!ctx) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": ctx is null");                         // nothing has been launched so far
    if (ctx->collective) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": the context carries a communicator; this call is single-GPU");
    ctx->anms_kernel_ms = 0.0;
    const int32_t total = kp_ptr[num_frames];
    for (int32_t f = 0; f <= num_frames; f++) keep_ptr[f] = 0;
    if (total == 0) return SSFM_OK;
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<AnmsItem> items;
    const int64_t split_items = anms_plan(num_frames, kp_ptr, num_to_keep, opt ? opt->force_j_chunks : 0, ctx->num_cus, items);
    if (items.size() > (size_t)0x7FFFFFFF) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": too many work items");
    std::vector<AnmsFrameDev> frames((size_t)num_frames);
    for (int32_t f = 0; f < num_frames; f++) frames[(size_t)f] = AnmsFrameDev{kp_ptr[f], kp_ptr[f + 1] - kp_ptr[f], num_to_keep[f], 0};
    std::vector<float> hxy(xy, xy + 2 * (size_t)total), hr(response, response + (size_t)total);
    DevBuf<float> d_xy, d_resp; DevBuf<AnmsItem> d_items; DevBuf<AnmsFrameDev> d_frames; DevBuf<unsigned long long> d_d2; DevBuf<int> d_rank, d_slot, d_keep, d_count;
    DevBuf<double> d_radius;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto release = [&]() {
        d_xy.free(); d_resp.free(); d_items.free(); d_frames.free(); d_d2.free(); d_rank.free(); d_slot.free(); d_keep.free(); d_count.free(); d_radius.free();
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        e0 = e1 = nullptr;
    };
    ANMS_CHECK(upload(d_xy, hxy, st)); ANMS_CHECK(upload(d_resp, hr, st)); ANMS_CHECK(upload(d_items, items, st)); ANMS_CHECK(upload(d_frames, frames, st));
    ANMS_CHECK(d_d2.alloc((size_t)total)); ANMS_CHECK(d_rank.alloc((size_t)total)); ANMS_CHECK(d_slot.alloc((size_t)total)); ANMS_CHECK(d_keep.alloc((size_t)total));
    ANMS_CHECK(d_count.alloc((size_t)num_frames)); ANMS_CHECK(d_radius.alloc((size_t)total));
    ANMS_CHECK(hipEventCreate(&e0)); ANMS_CHECK(hipEventCreate(&e1));
    ANMS_CHECK(hipEventRecord(e0, st));
    if (split_items > 0)
        hipLaunchKernelGGL(k_anms_init, dim3((unsigned)(((size_t)total + 255) / 256)), dim3(256), 0, st, total, d_d2.p, d_rank.p);
    if (!items.empty())
        hipLaunchKernelGGL(k_anms_radius, dim3((unsigned)items.size()), dim3(kAnmsBlock), 0, st, d_items.p, (const float2*)d_xy.p, d_resp.p, d_d2.p, d_rank.p);
    hipLaunchKernelGGL(k_anms_select, dim3((unsigned)num_frames), dim3(kAnmsSelectThreads), 0, st, d_frames.p, d_d2.p, d_rank.p, d_radius.p, d_slot.p, d_keep.p, d_count.p);
    ANMS_CHECK(hipGetLastError());
    ANMS_CHECK(hipEventRecord(e1, st));
    std::vector<int> hkeep((size_t)total), hcount((size_t)num_frames);
    ANMS_CHECK(hipMemcpyAsync(hkeep.data(), d_keep.p, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st));
    ANMS_CHECK(hipMemcpyAsync(hcount.data(), d_count.p, (size_t)num_frames * sizeof(int), hipMemcpyDeviceToHost, st));
    if (radius) ANMS_CHECK(hipMemcpyAsync(radius, d_radius.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st));
    ANMS_CHECK(hipStreamSynchronize(st));
    { float ms = 0.f; if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ctx->anms_kernel_ms = ms; else (void)hipGetLastError(); }
    for (int32_t f = 0; f < num_frames; f++) {
        const int32_t n = kp_ptr[f + 1] - kp_ptr[f], c = std::min(std::max(hcount[(size_t)f], 0), n);
        std::copy(hkeep.begin() + kp_ptr[f], hkeep.begin() + kp_ptr[f] + c, keep_idx + keep_ptr[f]);
        keep_ptr[f + 1] = keep_ptr[f] + c;
    }
    release();
    return SSFM_OK;
}
