// spherical_sfm_amd -- brute-force descriptor matching on the device: match() / match_exhaustive()
// (reference examples/spherical_sfm_tools.cpp:235-251 and :575-600; cv::BFMatcher::knnMatch(query, train, 2) + Lowe's ratio test + a std::map).
//
// Per pair (train = frame0, query = frame1):  for every query i its nearest (j1) and second nearest (j2) train by L2 distance;
// if (double)dist1 < ratio * (double)dist2 then m01[j1] = i, later queries overwriting earlier ones.
//
//   k_desc_norms    |t|^2 of every descriptor, once per call
//   k_match_dist    one workgroup per (pair, tile of 128 queries): the query tile stays in LDS, train tiles of 128 rows stream through a second LDS
//                   image (the next tile is in flight in registers while this one is multiplied).  T . Q^T on v_mfma_f32_32x32x2_f32 -- exact f32,
//                   a k-ordered fmaf chain -- with the TRAIN rows as the A operand: an accumulator lane then owns ONE query (column) and 16 train rows
//                   per 32x32 tile, so the running (best, second best) per query is kept in that lane's registers with no cross-lane traffic and the
//                   n1 x n0 distance matrix is never written.  Candidates are ranked by |t|^2 - 2 q.t (|q|^2 is common to a query's candidates).
//                   After the last train tile the partial lists of a query (2 lane halves x 2 waves) are merged through LDS, its two finalists are
//                   re-evaluated as sum (q - t)^2 in f32 -- the reference's form, so the cancellation of the product form never decides the ratio
//                   test -- and the test is made on sqrtf values in double, as the reference's float * double comparison does.
//   k_guided_dist   guided matching (ssfm_guided_match_pairs): k_match_dist with the epipolar band of the pair's E as a mask before the ranking; see the kernel
//   k_match_count / k_match_scan / k_match_compact
//                   atomicMax of the query index into the train's slot is "the last query wins" without any ordering; the slots of a pair are
//                   compacted into (j, i) lists in ascending j.  Nothing here depends on the order in which workgroups run: same bits every run.
//
// Exactness for SIFT input (floats holding integers 0..255): every partial sum is an integer below 2^24, so the product form is exact in any
// summation order and the lists equal those of any correct implementation.  Defined here where the reference is not: a train frame with fewer than
// two features yields no matches; equal distances rank the lower train index first (only visible with ratio >= 1).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "ssfm_ctx.h"
#include "knobs.h"
#include "pairwise_front.h"

namespace ssfm {

constexpr int MT = 128;            // tile edge (queries and train rows per tile)
constexpr int MK = 128;            // largest descriptor length
constexpr int MLD = MK + 4;        // LDS row stride in floats: 528 B rows put 16 consecutive rows on 16 distinct groups of 4 banks (ds_read_b128, 64 banks)

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MatchPair { int off0, n0, off1, n1; };      // feature offsets / counts of the train (0) and query (1) frame

template <typename T>
struct MBuf {                      // device buffer from the context's recycling pool (ssfm_ctx.h: DevPool; given back only after the stream was synchronised)
    T* p = nullptr; size_t cap = 0; int dev = 0;
    hipError_t alloc(size_t count) {
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        (void)hipGetDevice(&dev);
        p = static_cast<T*>(g_dev_pool.take(bytes, dev, &cap));
        if (p) return hipSuccess;
        hipError_t e = hipMalloc((void**)&p, bytes); cap = bytes;
        if (e != hipSuccess) { (void)hipGetLastError(); g_dev_pool.drain(dev); e = hipMalloc((void**)&p, bytes); if (e != hipSuccess) { p = nullptr; cap = 0; } }
        return e;
    }
    void free() { if (p && !g_dev_pool.give(p, cap, dev)) (void)hipFree(p); p = nullptr; cap = 0; }
};

static __global__ void __launch_bounds__(256) k_desc_norms(int total, int dim, const float* __restrict__ descs, float* __restrict__ norms) {
    // 32 lanes per descriptor, a float4 each (dim <= 128)
    const int f = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 5), c = threadIdx.x & 31;
    float s = 0.0f;
    if (f < total && 4 * c < dim) {
        const float4 v = *reinterpret_cast<const float4*>(descs + (size_t)f * dim + 4 * c);
        s = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, v.w * v.w)));
    }
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 32);
    if (f < total && c == 0) norms[f] = s;
}

// rows [row0, row0 + 128) of a frame's descriptors (n rows at `base`), as 16 float4 per thread: thread t owns column chunk t & 31 of rows (t >> 5) + 8 i
__device__ __forceinline__ void tile_fetch(float4 (&r)[16], const float* __restrict__ base, int n, int row0, int dim, int t) {
    const int c4 = t & 31;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int row = row0 + (t >> 5) + 8 * i;
        r[i] = (row < n && 4 * c4 < dim) ? *reinterpret_cast<const float4*>(base + (size_t)row * dim + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
__device__ __forceinline__ void tile_store(float* __restrict__ lds, const float4 (&r)[16], int t) {
#pragma unroll
    for (int i = 0; i < 16; i++) *reinterpret_cast<float4*>(lds + ((t >> 5) + 8 * i) * MLD + 4 * (t & 31)) = r[i];
}

// (s, j) ranks before (s', j') when s < s', or s == s' and j < j'
__device__ __forceinline__ bool ranks_before(float s, int j, float s2, int j2) { return s < s2 || (s == s2 && (unsigned)j < (unsigned)j2); }

// slots != nullptr: the ratio test + atomicMax of the query index into slots[pair * slot_stride + j1]
// nn != nullptr (probe, one pair): nn[2 i] = {j1, j2}, dist[2 i] = {dist1, dist2} of query i
static __global__ void __launch_bounds__(256)
k_match_dist(const MatchPair* __restrict__ pairs, const float* __restrict__ descs, const float* __restrict__ norms, int dim, double ratio,
             int* __restrict__ slots, int slot_stride, int* __restrict__ nn, float* __restrict__ dist) {
    __shared__ __attribute__((aligned(16))) float Qs[MT * MLD];
    __shared__ __attribute__((aligned(16))) float Ts[MT * MLD];
    __shared__ float tn[MT];
    __shared__ float cand_s[MT][8];
    __shared__ int cand_j[MT][8];
    const MatchPair P = pairs[blockIdx.y];
    const int q0 = blockIdx.x * MT;
    if (q0 >= P.n1) return;                                        // (uniform over the workgroup)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5, l31 = lane & 31;
    const int wr = wave >> 1, wc = wave & 1;                        // the wave's 64 train rows x 64 queries of the 128 x 128 tile
    const float* __restrict__ qbase = descs + (size_t)P.off1 * dim;
    const float* __restrict__ tbase = descs + (size_t)P.off0 * dim;
    const float INF = __builtin_inff();
    float4 pf[16];
    tile_fetch(pf, qbase, P.n1, q0, dim, t);
    tile_store(Qs, pf, t);
    tile_fetch(pf, tbase, P.n0, 0, dim, t);
    float pn = (t < MT) ? ((t < P.n0) ? norms[P.off0 + t] : INF) : 0.f;
    float b1[2] = {INF, INF}, b2[2] = {INF, INF}; int j1[2] = {-1, -1}, j2[2] = {-1, -1};
    const int kchunks = (dim + 7) >> 3;                            // 8 k per chunk: lane half h multiplies k = 8 c + 4 h .. + 3 (columns dim .. 127 of the images are zero)
    const int ntiles = (P.n0 + MT - 1) / MT;
    for (int tile = 0; tile < ntiles; tile++) {
        __syncthreads();                                           // the previous tile has been read by every wave
        tile_store(Ts, pf, t);
        if (t < MT) tn[t] = pn;
        __syncthreads();
        if (tile + 1 < ntiles) {                                   // next tile: global loads in flight under the products
            tile_fetch(pf, tbase, P.n0, (tile + 1) * MT, dim, t);
            if (t < MT) pn = ((tile + 1) * MT + t < P.n0) ? norms[P.off0 + (tile + 1) * MT + t] : INF;
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int n = 0; n < 2; n++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;
        const float* ap = Ts + (wr * 64 + l31) * MLD + 4 * half;
        const float* bp = Qs + (wc * 64 + l31) * MLD + 4 * half;
        for (int c = 0; c < kchunks; c++) {
            const float4 a0 = *reinterpret_cast<const float4*>(ap + 8 * c), a1 = *reinterpret_cast<const float4*>(ap + 32 * MLD + 8 * c);
            const float4 q0v = *reinterpret_cast<const float4*>(bp + 8 * c), q1v = *reinterpret_cast<const float4*>(bp + 32 * MLD + 8 * c);
            const float a[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
            const float b[2][4] = {{q0v.x, q0v.y, q0v.z, q0v.w}, {q1v.x, q1v.y, q1v.z, q1v.w}};
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int m = 0; m < 2; m++)
#pragma unroll
                    for (int n = 0; n < 2; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][k], b[n][k], acc[m][n], 0, 0, 0);
        }
        // D[i][j]: column j (query) = lane & 31, row i (train) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5): ascending in r, so a strict < keeps the lower index on ties
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int row = wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const float s = fmaf(-2.0f, acc[m][n][r], tn[row]);           // padding rows: |t|^2 = +inf, never below a finite value
                    const int j = tile * MT + row;
                    if (s < b1[n]) { b2[n] = b1[n]; j2[n] = j1[n]; b1[n] = s; j1[n] = j; }
                    else if (s < b2[n]) { b2[n] = s; j2[n] = j; }
                }
    }
    // merge the four partial lists of every query: source = 2 * wr + half
#pragma unroll
    for (int n = 0; n < 2; n++) {
        const int q = wc * 64 + n * 32 + l31, src = 2 * wr + half;
        cand_s[q][2 * src] = b1[n]; cand_j[q][2 * src] = j1[n];
        cand_s[q][2 * src + 1] = b2[n]; cand_j[q][2 * src + 1] = j2[n];
    }
    __syncthreads();
    // two threads per query: both merge, thread `which` re-evaluates finalist `which` directly
    const int q = t >> 1, which = t & 1, qi = q0 + q;
    float s1 = INF, s2 = INF; int f1 = -1, f2 = -1;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float s = cand_s[q][e]; const int j = cand_j[q][e];
        if (j < 0) continue;
        if (f1 < 0 || ranks_before(s, j, s1, f1)) { s2 = s1; f2 = f1; s1 = s; f1 = j; }
        else if (f2 < 0 || ranks_before(s, j, s2, f2)) { s2 = s; f2 = j; }
    }
    const int mine = which ? f2 : f1;
    float d = INF;
    if (qi < P.n1 && mine >= 0) {
        const float* __restrict__ tp = tbase + (size_t)mine * dim;
        const float* qp = Qs + q * MLD;
        float sum = 0.f;
        for (int k = 0; k < dim; k += 4) {
            const float4 tv = *reinterpret_cast<const float4*>(tp + k); const float4 qv = *reinterpret_cast<const float4*>(qp + k);
            float e;
            e = qv.x - tv.x; sum = fmaf(e, e, sum); e = qv.y - tv.y; sum = fmaf(e, e, sum);
            e = qv.z - tv.z; sum = fmaf(e, e, sum); e = qv.w - tv.w; sum = fmaf(e, e, sum);
        }
        d = (float)sqrt((double)sum);                              // sqrt in double of a float, rounded once more: the correctly rounded sqrtf
    }
    const float dother = __shfl_xor(d, 1);
    if (which == 0 && qi < P.n1) {
        float d1 = d, d2 = dother;
        if (f2 >= 0 && ranks_before(d2, f2, d1, f1)) { const float x = d1; d1 = d2; d2 = x; const int y = f1; f1 = f2; f2 = y; }   // the direct form has the last word on the order
        if (nn) { nn[2 * qi] = f1; nn[2 * qi + 1] = f2; dist[2 * qi] = d1; dist[2 * qi + 1] = d2; }
        if (slots && f2 >= 0 && (double)d1 < ratio * (double)d2) atomicMax(&slots[(size_t)blockIdx.y * slot_stride + f1], qi);
    }
}

// ---- guided matching (include/ssfm.h: ssfm_guided_match_pairs) ----------------------------------------------------------------------------------
// cand(i, j) of the header with  q = (v_i, a.x^2 + a.y^2),  b = (E u_j, b.x^2 + b.y^2):  fp64, no division; a NaN operand (padding rows) or 0 < 0 is "no"
__device__ __forceinline__ bool guided_cand(const double4& q, const double4& b, double thr2) {
    const double d = q.x * b.x + q.y * b.y + q.z * b.z;
    return d * d < thr2 * (b.w + q.w);
}

// k_match_dist with the epipolar band of the pair's E as a mask BEFORE the ranking: the same tiling, operands and running (best, second) per query; an entry whose
// predicate fails is skipped.  Per staged train tile threads 0..127 write (E u_j, b.x^2 + b.y^2) of their row into Tb, once per workgroup (E^T v_i -> v_i, a.x^2 + a.y^2)
// of the 128 queries into Qa; a lane keeps the records of its two queries in registers and reads a row's 32 B as a broadcast (two addresses per wave).
// MODE: where the predicate is evaluated (measured, DESIGN.md 4 "Guided matching"; the lab build selects with SSFM_GUIDED_MODE, the product has GUIDED_MODE only)
//   0  in the epilogue, only for an entry that would enter the lane's list (s < second best && cand): the same list, the fp64 part for a small share of entries
//   1  in the epilogue, for every entry, before the comparison (cand && s < second best)
//   2  for every entry in a loop of its own over the lane's 32 rows of the tile, packed into one bit mask per query that the epilogue tests
// COUNT = true (probe): cand_count[i] = the train rows inside the band of query i, from the masks of MODE 2.
// Acceptance: j1 exists, dist1 <= max_distance, and j2 is absent or (double)dist1 < ratio * (double)dist2.  E: 9 doubles per pair, column-major, v^T E u = 0.
constexpr int GUIDED_MODE = 2;
template <bool COUNT, int MODE = GUIDED_MODE>
static __global__ void __launch_bounds__(256)
k_guided_dist(const MatchPair* __restrict__ pairs, const float* __restrict__ descs, const float* __restrict__ norms, const double* __restrict__ rays,
              const double* __restrict__ Es, int dim, double ratio, double thr2, float max_distance, int* __restrict__ slots, int slot_stride,
              int* __restrict__ nn, float* __restrict__ dist, int* __restrict__ cand_count) {
    __shared__ __attribute__((aligned(16))) float Qs[MT * MLD];
    __shared__ __attribute__((aligned(16))) float Ts[MT * MLD];
    __shared__ float tn[MT];
    __shared__ float cand_s[MT][8];
    __shared__ int cand_j[MT][8];
    __shared__ __attribute__((aligned(32))) double4 Tb[MT];
    __shared__ __attribute__((aligned(32))) double4 Qa[MT];
    __shared__ int cand_c[MT][4];
    static_assert(!COUNT || MODE == 2, "the probe counts from the masks");
    const MatchPair P = pairs[blockIdx.y];
    const int q0 = blockIdx.x * MT;
    if (q0 >= P.n1) return;                                        // (uniform over the workgroup)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5, l31 = lane & 31;
    const int wr = wave >> 1, wc = wave & 1;
    const float* __restrict__ qbase = descs + (size_t)P.off1 * dim;
    const float* __restrict__ tbase = descs + (size_t)P.off0 * dim;
    const double* __restrict__ urays = rays + (size_t)P.off0 * 3;
    const float INF = __builtin_inff();
    const double QNAN = __builtin_nan("");
    double e[9];
#pragma unroll
    for (int k = 0; k < 9; k++) e[k] = Es[(size_t)blockIdx.y * 9 + k];
    float4 pf[16];
    tile_fetch(pf, qbase, P.n1, q0, dim, t);
    tile_store(Qs, pf, t);
    if (t < MT) {                                                  // a = E^T v: a[c] = sum_r E(r, c) v[r]
        double4 rec = make_double4(QNAN, QNAN, QNAN, QNAN);
        if (q0 + t < P.n1) {
            const double* __restrict__ v = rays + ((size_t)P.off1 + q0 + t) * 3;
            const double v0 = v[0], v1 = v[1], v2 = v[2];
            const double ax = e[0] * v0 + e[1] * v1 + e[2] * v2, ay = e[3] * v0 + e[4] * v1 + e[5] * v2;
            rec = make_double4(v0, v1, v2, ax * ax + ay * ay);
        }
        Qa[t] = rec;
    }
    tile_fetch(pf, tbase, P.n0, 0, dim, t);
    float pn = (t < MT) ? ((t < P.n0) ? norms[P.off0 + t] : INF) : 0.f;
    double pu[3] = {QNAN, QNAN, QNAN};
    if (t < MT && t < P.n0) { pu[0] = urays[3 * t]; pu[1] = urays[3 * t + 1]; pu[2] = urays[3 * t + 2]; }
    float b1[2] = {INF, INF}, b2[2] = {INF, INF}; int j1[2] = {-1, -1}, j2[2] = {-1, -1}, cnt[2] = {0, 0};
    const int kchunks = (dim + 7) >> 3;
    const int ntiles = (P.n0 + MT - 1) / MT;
    double4 vq[2] = {make_double4(QNAN, QNAN, QNAN, QNAN), make_double4(QNAN, QNAN, QNAN, QNAN)};
    for (int tile = 0; tile < ntiles; tile++) {
        __syncthreads();                                           // the previous tile has been read by every wave
        tile_store(Ts, pf, t);
        if (t < MT) {                                              // b = E u: b[r] = sum_c E(r, c) u[c]; a padding row holds NaN and is inside no band
            tn[t] = pn;
            const double bx = e[0] * pu[0] + e[3] * pu[1] + e[6] * pu[2], by = e[1] * pu[0] + e[4] * pu[1] + e[7] * pu[2], bz = e[2] * pu[0] + e[5] * pu[1] + e[8] * pu[2];
            Tb[t] = make_double4(bx, by, bz, bx * bx + by * by);
        }
        __syncthreads();
        if (tile == 0) { vq[0] = Qa[wc * 64 + l31]; vq[1] = Qa[wc * 64 + 32 + l31]; }
        if (tile + 1 < ntiles) {                                   // next tile: global loads in flight under the products
            tile_fetch(pf, tbase, P.n0, (tile + 1) * MT, dim, t);
            if (t < MT) {
                const int row = (tile + 1) * MT + t;
                pn = (row < P.n0) ? norms[P.off0 + row] : INF;
                if (row < P.n0) { pu[0] = urays[3 * (size_t)row]; pu[1] = urays[3 * (size_t)row + 1]; pu[2] = urays[3 * (size_t)row + 2]; }
                else { pu[0] = QNAN; pu[1] = QNAN; pu[2] = QNAN; }
            }
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int n = 0; n < 2; n++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;
        const float* ap = Ts + (wr * 64 + l31) * MLD + 4 * half;
        const float* bp = Qs + (wc * 64 + l31) * MLD + 4 * half;
        for (int c = 0; c < kchunks; c++) {
            const float4 a0 = *reinterpret_cast<const float4*>(ap + 8 * c), a1 = *reinterpret_cast<const float4*>(ap + 32 * MLD + 8 * c);
            const float4 q0v = *reinterpret_cast<const float4*>(bp + 8 * c), q1v = *reinterpret_cast<const float4*>(bp + 32 * MLD + 8 * c);
            const float a[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
            const float b[2][4] = {{q0v.x, q0v.y, q0v.z, q0v.w}, {q1v.x, q1v.y, q1v.z, q1v.w}};
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int m = 0; m < 2; m++)
#pragma unroll
                    for (int n = 0; n < 2; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][k], b[n][k], acc[m][n], 0, 0, 0);
        }
        unsigned in_mask[2] = {0u, 0u};                                // bit 16 m + r of query n = the predicate of the lane's 32 rows of this tile
        if (MODE == 2) {
#pragma unroll 4
            for (int k = 0; k < 32; k++) {
                const double4 bt = Tb[wr * 64 + (k >> 4) * 32 + (k & 3) + 8 * ((k & 15) >> 2) + 4 * half];
                in_mask[0] |= (unsigned)guided_cand(vq[0], bt, thr2) << k;
                in_mask[1] |= (unsigned)guided_cand(vq[1], bt, thr2) << k;
            }
            if (COUNT) { cnt[0] += __popc(in_mask[0]); cnt[1] += __popc(in_mask[1]); }
        }
        // rows ascend in (m, r): a strict < keeps the lower index on ties among the entries inside the band
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int row = wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const float s = fmaf(-2.0f, acc[m][n][r], tn[row]);           // padding rows: |t|^2 = +inf, never below a finite value
                    const int j = tile * MT + row;
                    if (MODE == 2 ? (((in_mask[n] >> (16 * m + r)) & 1u) && s < b2[n])
                                  : MODE == 1 ? (guided_cand(vq[n], Tb[row], thr2) && s < b2[n]) : (s < b2[n] && guided_cand(vq[n], Tb[row], thr2))) {
                        if (s < b1[n]) { b2[n] = b1[n]; j2[n] = j1[n]; b1[n] = s; j1[n] = j; }
                        else { b2[n] = s; j2[n] = j; }
                    }
                }
    }
    // merge the four partial lists of every query: source = 2 * wr + half
#pragma unroll
    for (int n = 0; n < 2; n++) {
        const int q = wc * 64 + n * 32 + l31, src = 2 * wr + half;
        cand_s[q][2 * src] = b1[n]; cand_j[q][2 * src] = j1[n];
        cand_s[q][2 * src + 1] = b2[n]; cand_j[q][2 * src + 1] = j2[n];
        if (COUNT) cand_c[q][src] = cnt[n];
    }
    __syncthreads();
    // two threads per query: both merge, thread `which` re-evaluates finalist `which` directly
    const int q = t >> 1, which = t & 1, qi = q0 + q;
    float s1 = INF, s2 = INF; int f1 = -1, f2 = -1;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float s = cand_s[q][k]; const int j = cand_j[q][k];
        if (j < 0) continue;
        if (f1 < 0 || ranks_before(s, j, s1, f1)) { s2 = s1; f2 = f1; s1 = s; f1 = j; }
        else if (f2 < 0 || ranks_before(s, j, s2, f2)) { s2 = s; f2 = j; }
    }
    const int mine = which ? f2 : f1;
    float d = INF;
    if (qi < P.n1 && mine >= 0) {
        const float* __restrict__ tp = tbase + (size_t)mine * dim;
        const float* qp = Qs + q * MLD;
        float sum = 0.f;
        for (int k = 0; k < dim; k += 4) {
            const float4 tv = *reinterpret_cast<const float4*>(tp + k); const float4 qv = *reinterpret_cast<const float4*>(qp + k);
            float x;
            x = qv.x - tv.x; sum = fmaf(x, x, sum); x = qv.y - tv.y; sum = fmaf(x, x, sum);
            x = qv.z - tv.z; sum = fmaf(x, x, sum); x = qv.w - tv.w; sum = fmaf(x, x, sum);
        }
        d = (float)sqrt((double)sum);                              // the correctly rounded sqrtf, as in k_match_dist
    }
    const float dother = __shfl_xor(d, 1);
    if (which == 0 && qi < P.n1) {
        float d1 = d, d2 = dother;
        if (f2 >= 0 && ranks_before(d2, f2, d1, f1)) { const float x = d1; d1 = d2; d2 = x; const int y = f1; f1 = f2; f2 = y; }   // the direct form has the last word on the order
        if (nn) { nn[2 * qi] = f1; nn[2 * qi + 1] = f2; dist[2 * qi] = d1; dist[2 * qi + 1] = d2; }
        if (COUNT && cand_count) cand_count[qi] = cand_c[q][0] + cand_c[q][1] + cand_c[q][2] + cand_c[q][3];
        if (slots && f1 >= 0 && d1 <= max_distance && (f2 < 0 || (double)d1 < ratio * (double)d2)) atomicMax(&slots[(size_t)blockIdx.y * slot_stride + f1], qi);
    }
}

static __global__ void __launch_bounds__(256) k_match_count(const MatchPair* __restrict__ pairs, const int* __restrict__ slots, int slot_stride, int* __restrict__ counts) {
    const int p = blockIdx.x, n0 = pairs[p].n0;
    int c = 0;
    for (int j = threadIdx.x; j < n0; j += 256) c += slots[(size_t)p * slot_stride + j] >= 0;
    int total; (void)block_exclusive_scan(c, &total);
    if (threadIdx.x == 0) counts[p] = total;
}

// ptr[0 .. np]: exclusive scan of counts (one workgroup; np is a few thousand)
static __global__ void __launch_bounds__(256) k_match_scan(int np, const int* __restrict__ counts, int* __restrict__ ptr) {
    int carry = 0;
    for (int b = 0; b < np; b += 256) {
        const int i = b + threadIdx.x, v = i < np ? counts[i] : 0;
        int total; const int ex = block_exclusive_scan(v, &total);
        if (i < np) ptr[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) ptr[np] = carry;
}

static __global__ void __launch_bounds__(256) k_match_compact(const MatchPair* __restrict__ pairs, const int* __restrict__ slots, int slot_stride, const int* __restrict__ ptr,
                                                       int* __restrict__ idx0, int* __restrict__ idx1) {
    const int p = blockIdx.x, n0 = pairs[p].n0;
    int base = ptr[p];
    for (int b = 0; b < n0; b += 256) {
        const int j = b + threadIdx.x, i = j < n0 ? slots[(size_t)p * slot_stride + j] : -1;
        int total; const int ex = block_exclusive_scan(i >= 0, &total);
        if (i >= 0) { idx0[base + ex] = j; idx1[base + ex] = i; }
        base += total;
    }
}

struct MatchDevice {               // everything a call owns on the device
    MBuf<float> descs, norms, pdist; MBuf<MatchPair> pairs; MBuf<int> slots, counts, ptr, idx0, idx1, pnn, pcnt;
    MBuf<double> rays, E;          // guided matching only
    hipEvent_t e0 = nullptr, e1 = nullptr;
    void release() {
        descs.free(); norms.free(); pdist.free(); pairs.free(); slots.free(); counts.free(); ptr.free(); idx0.free(); idx1.free(); pnn.free(); pcnt.free();
        rays.free(); E.free();
        if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); e0 = e1 = nullptr;
    }
};

static int upload_descs(ssfm_ctx* ctx, MatchDevice& D, size_t total, int dim, const float* descs) {
    SSFM_HIP_CHECK(ctx, D.descs.alloc(total * dim)); SSFM_HIP_CHECK(ctx, D.norms.alloc(total));
    if (total) {
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(D.descs.p, descs, total * dim * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_desc_norms, dim3((unsigned)((total * 32 + 255) / 256)), dim3(256), 0, ctx->stream, (int)total, dim, D.descs.p, D.norms.p);
        SSFM_HIP_CHECK(ctx, hipGetLastError());
    }
    return SSFM_OK;
}

static bool dim_ok(int dim) { return dim >= 4 && dim <= MK && dim % 4 == 0; }

int match_check_args(ssfm_ctx* ctx, const char* who, int32_t num_frames, const int32_t* feat_ptr, const float* descs, int32_t num_pairs, const int32_t* pair_frame0,
                     const int32_t* pair_frame1, const ssfm_match_options* opt, ssfm_match_options* O) {
    const std::string w(who);
    if (num_frames <= 0 || !feat_ptr || num_pairs < 0 || (num_pairs > 0 && (!pair_frame0 || !pair_frame1)))
        return fail(ctx, SSFM_ERR_INVALID, w + ": bad arguments (num_frames > 0, feat_ptr and the pair lists are required)");
    ssfm_match_default_options(O); if (opt) *O = *opt;
    if (!dim_ok(O->dim)) return fail(ctx, SSFM_ERR_INVALID, w + ": dim must be a multiple of 4 in 4..128");
    if (!(O->ratio > 0.0) || !std::isfinite(O->ratio)) return fail(ctx, SSFM_ERR_INVALID, w + ": ratio must be positive and finite");
    if (feat_ptr[0] != 0) return fail(ctx, SSFM_ERR_INVALID, w + ": feat_ptr[0] must be 0");
    for (int f = 0; f < num_frames; f++) if (feat_ptr[f + 1] < feat_ptr[f]) return fail(ctx, SSFM_ERR_INVALID, w + ": feat_ptr must ascend");
    if (feat_ptr[num_frames] && !descs) return fail(ctx, SSFM_ERR_INVALID, w + ": descs is null");
    for (int p = 0; p < num_pairs; p++) {
        const int f0 = pair_frame0[p], f1 = pair_frame1[p];
        if (f0 < 0 || f0 >= num_frames || f1 < 0 || f1 >= num_frames) return fail(ctx, SSFM_ERR_INVALID, w + ": frame index out of range");
    }
    return SSFM_OK;
}

// what ssfm_guided_match_pairs adds to a run of the slab loop: the rays of all features, one E per pair (host pointers) and the rule's constants
struct GuidedArgs { const double* rays; const double* E; double thr2; float max_distance; };

// the slab loop of ssfm_match_pairs; with G the distance kernel is k_guided_dist and the time goes to ctx->guided_kernel_ms
static int match_slabs_impl(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, int32_t num_pairs, const int32_t* pair_frame0,
                            const int32_t* pair_frame1, const ssfm_match_options& O, const GuidedArgs* G, const MatchSlabSink& sink) {
    double& kernel_ms = G ? ctx->guided_kernel_ms : ctx->match_kernel_ms;
    const size_t total = (size_t)feat_ptr[num_frames];
    int max_n0 = 1;
    for (int p = 0; p < num_pairs; p++) max_n0 = std::max(max_n0, feat_ptr[pair_frame0[p] + 1] - feat_ptr[pair_frame0[p]]);
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    kernel_ms = 0.0;
    if (num_pairs == 0) return SSFM_OK;
    // slabs: the slot buffer (pairs of the slab x max n0 x 4 B) stays within 64 MB; SSFM_MATCH_SLAB_PAIRS (read at every call) overrides the pair count
    int slab_pairs = (int)std::min<size_t>(32768, std::max<size_t>(1, ((size_t)16 << 20) / (size_t)max_n0));
    if (const char* e = getenv("SSFM_MATCH_SLAB_PAIRS")) slab_pairs = std::min(32768, std::max(atoi(e), 1));
    slab_pairs = std::min(slab_pairs, num_pairs);
    hipStream_t st = ctx->stream;
    MatchDevice D;
    std::vector<MatchPair> hp((size_t)slab_pairs); std::vector<int> hptr((size_t)slab_pairs + 1);
    auto body = [&]() -> int {
        { const int r = upload_descs(ctx, D, total, O.dim, descs); if (r) return r; }
        if (G) {
            SSFM_HIP_CHECK(ctx, D.rays.alloc(total * 3)); SSFM_HIP_CHECK(ctx, D.E.alloc((size_t)num_pairs * 9));
            if (total) SSFM_HIP_CHECK(ctx, hipMemcpyAsync(D.rays.p, G->rays, total * 3 * sizeof(double), hipMemcpyHostToDevice, st));
            SSFM_HIP_CHECK(ctx, hipMemcpyAsync(D.E.p, G->E, (size_t)num_pairs * 9 * sizeof(double), hipMemcpyHostToDevice, st));
        }
        const size_t nslot = (size_t)slab_pairs * max_n0;
        SSFM_HIP_CHECK(ctx, D.pairs.alloc(slab_pairs)); SSFM_HIP_CHECK(ctx, D.slots.alloc(nslot)); SSFM_HIP_CHECK(ctx, D.counts.alloc(slab_pairs));
        SSFM_HIP_CHECK(ctx, D.ptr.alloc((size_t)slab_pairs + 1)); SSFM_HIP_CHECK(ctx, D.idx0.alloc(nslot)); SSFM_HIP_CHECK(ctx, D.idx1.alloc(nslot));
        SSFM_HIP_CHECK(ctx, hipEventCreate(&D.e0)); SSFM_HIP_CHECK(ctx, hipEventCreate(&D.e1));
        for (int p0 = 0; p0 < num_pairs; p0 += slab_pairs) {
            const int np = std::min(slab_pairs, num_pairs - p0);
            int max_n1 = 0;
            for (int i = 0; i < np; i++) {
                const int f0 = pair_frame0[p0 + i], f1 = pair_frame1[p0 + i];
                hp[i] = MatchPair{feat_ptr[f0], feat_ptr[f0 + 1] - feat_ptr[f0], feat_ptr[f1], feat_ptr[f1 + 1] - feat_ptr[f1]};
                max_n1 = std::max(max_n1, hp[i].n1);
            }
            SSFM_HIP_CHECK(ctx, hipMemcpyAsync(D.pairs.p, hp.data(), (size_t)np * sizeof(MatchPair), hipMemcpyHostToDevice, st));
            SSFM_HIP_CHECK(ctx, hipMemsetAsync(D.slots.p, 0xFF, (size_t)np * max_n0 * sizeof(int), st));      // every slot -1
            SSFM_HIP_CHECK(ctx, hipEventRecord(D.e0, st));
#ifdef SSFM_LAB
            if (max_n1 > 0 && G && SSFM_LAB_KNOB("SSFM_GUIDED_MODE", GUIDED_MODE) == 0)
                hipLaunchKernelGGL((k_guided_dist<false, 0>), dim3((max_n1 + MT - 1) / MT, np), dim3(256), 0, st, D.pairs.p, D.descs.p, D.norms.p, D.rays.p, D.E.p + (size_t)p0 * 9,
                                   O.dim, O.ratio, G->thr2, G->max_distance, D.slots.p, max_n0, (int*)nullptr, (float*)nullptr, (int*)nullptr);
            else if (max_n1 > 0 && G && SSFM_LAB_KNOB("SSFM_GUIDED_MODE", GUIDED_MODE) == 1)
                hipLaunchKernelGGL((k_guided_dist<false, 1>), dim3((max_n1 + MT - 1) / MT, np), dim3(256), 0, st, D.pairs.p, D.descs.p, D.norms.p, D.rays.p, D.E.p + (size_t)p0 * 9,
                                   O.dim, O.ratio, G->thr2, G->max_distance, D.slots.p, max_n0, (int*)nullptr, (float*)nullptr, (int*)nullptr);
            else
#endif
            if (max_n1 > 0 && G)
                hipLaunchKernelGGL(k_guided_dist<false>, dim3((max_n1 + MT - 1) / MT, np), dim3(256), 0, st, D.pairs.p, D.descs.p, D.norms.p, D.rays.p, D.E.p + (size_t)p0 * 9,
                                   O.dim, O.ratio, G->thr2, G->max_distance, D.slots.p, max_n0, (int*)nullptr, (float*)nullptr, (int*)nullptr);
            else if (max_n1 > 0)
                hipLaunchKernelGGL(k_match_dist, dim3((max_n1 + MT - 1) / MT, np), dim3(256), 0, st, D.pairs.p, D.descs.p, D.norms.p, O.dim, O.ratio, D.slots.p, max_n0,
                                   (int*)nullptr, (float*)nullptr);
            hipLaunchKernelGGL(k_match_count, dim3(np), dim3(256), 0, st, D.pairs.p, D.slots.p, max_n0, D.counts.p);
            hipLaunchKernelGGL(k_match_scan, dim3(1), dim3(256), 0, st, np, D.counts.p, D.ptr.p);
            hipLaunchKernelGGL(k_match_compact, dim3(np), dim3(256), 0, st, D.pairs.p, D.slots.p, max_n0, D.ptr.p, D.idx0.p, D.idx1.p);
            SSFM_HIP_CHECK(ctx, hipGetLastError());
            SSFM_HIP_CHECK(ctx, hipEventRecord(D.e1, st));
            SSFM_HIP_CHECK(ctx, hipMemcpyAsync(hptr.data(), D.ptr.p, ((size_t)np + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
            SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
            { float ms = 0.f; if (hipEventElapsedTime(&ms, D.e0, D.e1) == hipSuccess) kernel_ms += ms; else (void)hipGetLastError(); }
            { const int r = sink(p0, np, hptr.data(), D.idx0.p, D.idx1.p); if (r) return r; }
        }
        return SSFM_OK;
    };
    const int rc = body();
    (void)hipStreamSynchronize(st);
    D.release();
    return rc;
}

int match_slabs(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, int32_t num_pairs, const int32_t* pair_frame0,
                const int32_t* pair_frame1, const ssfm_match_options& O, const MatchSlabSink& sink) {
    return match_slabs_impl(ctx, num_frames, feat_ptr, descs, num_pairs, pair_frame0, pair_frame1, O, nullptr, sink);
}

}  // namespace ssfm

using namespace ssfm;

extern "C" void ssfm_match_default_options(ssfm_match_options* o) {
    if (!o) return;
    o->ratio = 0.75; o->dim = 128; o->reserved = 0;
}

extern "C" int ssfm_match_last_kernel_ms(ssfm_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SSFM_ERR_INVALID;
    *ms = ctx->match_kernel_ms;
    return SSFM_OK;
}

extern "C" int ssfm_match_pairs(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, int32_t num_pairs, const int32_t* pair_frame0,
                                const int32_t* pair_frame1, const ssfm_match_options* opt, int64_t capacity, int32_t* match_ptr, int32_t* match_idx0,
                                int32_t* match_idx1) {
    if (!ctx) return SSFM_ERR_INVALID;
    if (num_frames <= 0 || !feat_ptr || num_pairs < 0 || (num_pairs > 0 && (!pair_frame0 || !pair_frame1)) || !match_ptr || capacity < 0)
        return fail(ctx, SSFM_ERR_INVALID, "ssfm_match_pairs: bad arguments (num_frames > 0, feat_ptr, the pair lists and match_ptr are required)");
    if ((match_idx0 == nullptr) != (match_idx1 == nullptr)) return fail(ctx, SSFM_ERR_INVALID, "ssfm_match_pairs: match_idx0 and match_idx1 are given together or not at all");
    ssfm_match_options O;
    { const int r = match_check_args(ctx, "ssfm_match_pairs", num_frames, feat_ptr, descs, num_pairs, pair_frame0, pair_frame1, opt, &O); if (r) return r; }
    match_ptr[0] = 0;
    hipStream_t st = ctx->stream;
    int64_t running = 0; bool overflow = false;
    int rc = match_slabs(ctx, num_frames, feat_ptr, descs, num_pairs, pair_frame0, pair_frame1, O, [&](int p0, int np, const int* hptr, const int* d_idx0, const int* d_idx1) -> int {
        const int64_t slab_total = hptr[np];
        if (running + slab_total > (int64_t)std::numeric_limits<int32_t>::max()) return fail(ctx, SSFM_ERR_INVALID, "ssfm_match_pairs: more than INT32_MAX matches in one call");
        for (int i = 1; i <= np; i++) match_ptr[p0 + i] = (int32_t)(running + hptr[i]);
        if (match_idx0) {
            if (running + slab_total > capacity) overflow = true;      // keep counting: match_ptr[num_pairs] reports the capacity needed
            else if (slab_total) {
                SSFM_HIP_CHECK(ctx, hipMemcpyAsync(match_idx0 + running, d_idx0, (size_t)slab_total * sizeof(int), hipMemcpyDeviceToHost, st));
                SSFM_HIP_CHECK(ctx, hipMemcpyAsync(match_idx1 + running, d_idx1, (size_t)slab_total * sizeof(int), hipMemcpyDeviceToHost, st));
                SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
            }
        }
        running += slab_total;
        return SSFM_OK;
    });
    if (rc == SSFM_OK && overflow) rc = fail(ctx, SSFM_ERR_INVALID, "ssfm_match_pairs: capacity too small; match_ptr[num_pairs] holds the number of matches");
    return rc;
}

extern "C" int ssfm_match_knn_probe(ssfm_ctx* ctx, int32_t n0, const float* train, int32_t n1, const float* query, int32_t dim, int32_t* nn, float* dist) {
    if (!ctx) return SSFM_ERR_INVALID;
    if (n0 < 0 || n1 < 0 || (n0 > 0 && !train) || (n1 > 0 && !query) || !nn || !dist) return fail(ctx, SSFM_ERR_INVALID, "ssfm_match_knn_probe: bad arguments");
    if (!dim_ok(dim)) return fail(ctx, SSFM_ERR_INVALID, "ssfm_match_knn_probe: dim must be a multiple of 4 in 4..128");
    if ((size_t)n0 + (size_t)n1 > (size_t)std::numeric_limits<int32_t>::max()) return fail(ctx, SSFM_ERR_INVALID, "ssfm_match_knn_probe: too many descriptors");
    if (n1 == 0) return SSFM_OK;
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    MatchDevice D;
    std::vector<float> both(((size_t)n0 + n1) * dim);
    if (n0) std::memcpy(both.data(), train, (size_t)n0 * dim * sizeof(float));
    std::memcpy(both.data() + (size_t)n0 * dim, query, (size_t)n1 * dim * sizeof(float));
    const MatchPair P{0, n0, n0, n1};
    auto body = [&]() -> int {
        { const int r = upload_descs(ctx, D, (size_t)n0 + n1, dim, both.data()); if (r) return r; }
        SSFM_HIP_CHECK(ctx, D.pairs.alloc(1)); SSFM_HIP_CHECK(ctx, D.pnn.alloc((size_t)2 * n1)); SSFM_HIP_CHECK(ctx, D.pdist.alloc((size_t)2 * n1));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(D.pairs.p, &P, sizeof(P), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_match_dist, dim3((n1 + MT - 1) / MT, 1), dim3(256), 0, st, D.pairs.p, D.descs.p, D.norms.p, (int)dim, 1.0, (int*)nullptr, 0, D.pnn.p, D.pdist.p);
        SSFM_HIP_CHECK(ctx, hipGetLastError());
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(nn, D.pnn.p, (size_t)2 * n1 * sizeof(int), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(dist, D.pdist.p, (size_t)2 * n1 * sizeof(float), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        return SSFM_OK;
    };
    const int rc = body();
    (void)hipStreamSynchronize(st);
    D.release();
    return rc;
}

// ---- guided matching ------------------------------------------------------------------------------------------------------------------------------

extern "C" void ssfm_guided_match_default_options(ssfm_guided_match_options* o) {
    if (!o) return;
    o->ratio = 0.75; o->squared_threshold = 0.0; o->max_distance = std::numeric_limits<float>::infinity(); o->dim = 128;
}

extern "C" int ssfm_guided_match_last_kernel_ms(ssfm_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SSFM_ERR_INVALID;
    *ms = ctx->guided_kernel_ms;
    return SSFM_OK;
}

extern "C" int ssfm_guided_match_pairs(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, const double* feat_rays, int32_t num_pairs,
                                       const int32_t* pair_frame0, const int32_t* pair_frame1, const double* E, const ssfm_guided_match_options* opt, int64_t capacity,
                                       int32_t* match_ptr, int32_t* match_idx0, int32_t* match_idx1) {
    if (!ctx) return SSFM_ERR_INVALID;
    if (num_frames <= 0 || !feat_ptr || num_pairs < 0 || (num_pairs > 0 && (!pair_frame0 || !pair_frame1)) || !match_ptr || capacity < 0)
        return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_match_pairs: bad arguments (num_frames > 0, feat_ptr, the pair lists and match_ptr are required)");
    if ((match_idx0 == nullptr) != (match_idx1 == nullptr)) return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_match_pairs: match_idx0 and match_idx1 are given together or not at all");
    if (ctx->collective) return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_match_pairs: the context carries a communicator; this call is single-GPU");
    ssfm_guided_match_options GO; ssfm_guided_match_default_options(&GO); if (opt) GO = *opt;
    const ssfm_match_options MO{GO.ratio, GO.dim, 0};
    ssfm_match_options O;
    { const int r = match_check_args(ctx, "ssfm_guided_match_pairs", num_frames, feat_ptr, descs, num_pairs, pair_frame0, pair_frame1, &MO, &O); if (r) return r; }
    if (num_pairs > 0 && !E) return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_match_pairs: E is null");
    if (num_pairs > 0 && feat_ptr[num_frames] && !feat_rays) return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_match_pairs: feat_rays is null");
    if (!(GO.squared_threshold >= 0.0)) return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_match_pairs: squared_threshold must be >= 0");
    if (!(GO.max_distance >= 0.0f)) return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_match_pairs: max_distance must be >= 0");
    match_ptr[0] = 0;
    hipStream_t st = ctx->stream;
    const GuidedArgs G{feat_rays, E, GO.squared_threshold, GO.max_distance};
    int64_t running = 0; bool overflow = false;
    int rc = match_slabs_impl(ctx, num_frames, feat_ptr, descs, num_pairs, pair_frame0, pair_frame1, O, &G, [&](int p0, int np, const int* hptr, const int* d_idx0, const int* d_idx1) -> int {
        const int64_t slab_total = hptr[np];
        if (running + slab_total > (int64_t)std::numeric_limits<int32_t>::max()) return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_match_pairs: more than INT32_MAX matches in one call");
        for (int i = 1; i <= np; i++) match_ptr[p0 + i] = (int32_t)(running + hptr[i]);
        if (match_idx0) {
            if (running + slab_total > capacity) overflow = true;      // keep counting: match_ptr[num_pairs] reports the capacity needed
            else if (slab_total) {
                SSFM_HIP_CHECK(ctx, hipMemcpyAsync(match_idx0 + running, d_idx0, (size_t)slab_total * sizeof(int), hipMemcpyDeviceToHost, st));
                SSFM_HIP_CHECK(ctx, hipMemcpyAsync(match_idx1 + running, d_idx1, (size_t)slab_total * sizeof(int), hipMemcpyDeviceToHost, st));
                SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
            }
        }
        running += slab_total;
        return SSFM_OK;
    });
    if (rc == SSFM_OK && overflow) rc = fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_match_pairs: capacity too small; match_ptr[num_pairs] holds the number of matches");
    return rc;
}

extern "C" int ssfm_guided_knn_probe(ssfm_ctx* ctx, int32_t n0, const float* train, const double* u, int32_t n1, const float* query, const double* v, int32_t dim,
                                     const double* E, double squared_threshold, int32_t* nn, float* dist, int32_t* cand_count) {
    if (!ctx) return SSFM_ERR_INVALID;
    if (n0 < 0 || n1 < 0 || (n0 > 0 && (!train || !u)) || (n1 > 0 && (!query || !v)) || !E || !nn || !dist || !cand_count)
        return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_knn_probe: bad arguments");
    if (!dim_ok(dim)) return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_knn_probe: dim must be a multiple of 4 in 4..128");
    if (!(squared_threshold >= 0.0)) return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_knn_probe: squared_threshold must be >= 0");
    if ((size_t)n0 + (size_t)n1 > (size_t)std::numeric_limits<int32_t>::max()) return fail(ctx, SSFM_ERR_INVALID, "ssfm_guided_knn_probe: too many descriptors");
    if (n1 == 0) return SSFM_OK;
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    MatchDevice D;
    const size_t total = (size_t)n0 + n1;
    std::vector<float> both(total * dim); std::vector<double> rays(total * 3);
    if (n0) { std::memcpy(both.data(), train, (size_t)n0 * dim * sizeof(float)); std::memcpy(rays.data(), u, (size_t)n0 * 3 * sizeof(double)); }
    std::memcpy(both.data() + (size_t)n0 * dim, query, (size_t)n1 * dim * sizeof(float)); std::memcpy(rays.data() + (size_t)n0 * 3, v, (size_t)n1 * 3 * sizeof(double));
    const MatchPair P{0, n0, n0, n1};
    auto body = [&]() -> int {
        { const int r = upload_descs(ctx, D, total, dim, both.data()); if (r) return r; }
        SSFM_HIP_CHECK(ctx, D.pairs.alloc(1)); SSFM_HIP_CHECK(ctx, D.pnn.alloc((size_t)2 * n1)); SSFM_HIP_CHECK(ctx, D.pdist.alloc((size_t)2 * n1)); SSFM_HIP_CHECK(ctx, D.pcnt.alloc(n1));
        SSFM_HIP_CHECK(ctx, D.rays.alloc(total * 3)); SSFM_HIP_CHECK(ctx, D.E.alloc(9));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(D.pairs.p, &P, sizeof(P), hipMemcpyHostToDevice, st));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(D.rays.p, rays.data(), total * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(D.E.p, E, 9 * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_guided_dist<true>, dim3((n1 + MT - 1) / MT, 1), dim3(256), 0, st, D.pairs.p, D.descs.p, D.norms.p, D.rays.p, D.E.p, (int)dim, 1.0, squared_threshold,
                           std::numeric_limits<float>::infinity(), (int*)nullptr, 0, D.pnn.p, D.pdist.p, D.pcnt.p);
        SSFM_HIP_CHECK(ctx, hipGetLastError());
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(nn, D.pnn.p, (size_t)2 * n1 * sizeof(int), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(dist, D.pdist.p, (size_t)2 * n1 * sizeof(float), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(cand_count, D.pcnt.p, (size_t)n1 * sizeof(int), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        return SSFM_OK;
    };
    const int rc = body();
    (void)hipStreamSynchronize(st);
    D.release();
    return rc;
}
