// spherical_sfm_amd -- feature tracks of build_sfm (merge = true) as connected components of the match graph, on the device.  The contract is in
// include/ssfm.h (ssfm_build_tracks_device); the host bookkeeping it restates is tracks.cpp, which stays the default of both drivers.
//
// Global feature id g = feat_ptr[k] + local index.  parent[g] is a union-find forest with ONE invariant: parent[g] <= g, equality exactly at a root, and
// parent[g] is always a member of g's component.  It is written by a compare-and-swap that hooks a root under a smaller id and by atomicMin with an
// ancestor (compression): values only fall.  Every chase therefore walks strictly falling ids and ends; a component's root is its smallest member
// whatever the schedule, which is where the order independence of the whole call comes from.
//
//   k_tracks_init      parent = identity, touched = 0
//   k_tracks_link      a lane per match: its set by bisection of ms_ptr, g0 / g1 range-checked (a flag is raised, the match is skipped), both marked
//                      touched, union(g0, g1)
//   k_tracks_roots     root[g] by a chase (the forest is final: plain loads); flag = touched root; per-workgroup flag sums
//   k_tracks_scan_sums exclusive scan of the per-workgroup sums (one workgroup), the grand total to the counters
//   k_tracks_ids       id of a root = its position among the touched roots: ascending smallest member, 0 .. P-1
//   k_tracks_assign    tracks[g] = id[root[g]] or -1; (camera, track) -> smallest g in an open-addressing table (compare-and-swap on the key, atomicMin
//                      on the value), the slot remembered per feature
//   k_tracks_winners   a feature that is not the minimum of its slot flags its track as conflicted; winner flags and their per-workgroup sums
//   k_tracks_compact   winners in feature order -> (g, track)
// The camera, the local index and the pixel of an observation follow from g on the host, while the lists are copied out of the pinned staging: 8 bytes per
// match go up, 4 bytes per feature, 1 per point and 8 per observation come down.
// No lane waits for another lane's write, there is no lock, no flag that is spun on and no barrier between workgroups; the bound of every loop is stated at
// the loop.
#include <algorithm>
#include <cstring>
#include <string>
#include "pairwise_front.h"

namespace ssfm {

struct TrackSet { int off0, n0, off1, n1; };                        // first feature and feature count of the two frames of a match set
constexpr unsigned long long kTrackEmptyKey = ~0ull;               // (camera << 32 | track) never has its top bit set
constexpr int kTrackBlock = 256;

__device__ __forceinline__ int track_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x as this lane sees it, and the nodes passed get it as their parent unless they hold a smaller one already.
__device__ __forceinline__ int track_find(int* parent, int x) {
    int r = x;
    // bound: r strictly falls (the loop goes on only with p < r) and ids are >= 0: at most x steps
    for (;;) { const int p = track_load(parent + r); if (p >= r) break; r = p; }
    int y = x;
    // bound: y strictly falls (the loop goes on only with p < y) and stops at r: at most x - r steps.  r is an ancestor of every y passed, so
    // atomicMin(parent[y], r) keeps the invariant
    while (y > r) {
        const int p = track_load(parent + y);
        if (p > r) atomicMin(parent + y, r);
        if (p >= y) break;
        y = p;
    }
    return r;
}

// first index i in [0, n] with ptr[i] > v, minus one: the k with ptr[k] <= v < ptr[k + 1] (ptr ascending, ptr[0] <= v < ptr[n])
__device__ __forceinline__ int track_segment(const int* __restrict__ ptr, int n, int v) {
    int lo = 0, hi = n;                                            // ptr[lo] <= v < ptr[hi]
    // bound: hi - lo at least halves per step: at most 32 steps
    while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if (ptr[mid] <= v) lo = mid; else hi = mid; }
    return lo;
}

static __global__ void __launch_bounds__(kTrackBlock)
k_tracks_init(int total, int* __restrict__ parent, int* __restrict__ touched) {
    const int g = blockIdx.x * kTrackBlock + threadIdx.x;
    if (g < total) { parent[g] = g; touched[g] = 0; }
}

static __global__ void __launch_bounds__(kTrackBlock)
k_tracks_link(int num_matches, int num_sets, const int* __restrict__ ms_ptr, const TrackSet* __restrict__ sets, const int* __restrict__ f0,
              const int* __restrict__ f1, int* parent, int* __restrict__ touched, int* __restrict__ bad) {
    const int m = blockIdx.x * kTrackBlock + threadIdx.x;
    if (m >= num_matches) return;
    const TrackSet S = sets[track_segment(ms_ptr, num_sets, m)];
    const int l0 = f0[m], l1 = f1[m];
    if ((unsigned)l0 >= (unsigned)S.n0 || (unsigned)l1 >= (unsigned)S.n1) { *bad = 1; return; }       // (every writer stores the same value)
    const int g0 = S.off0 + l0, g1 = S.off1 + l1;
    touched[g0] = 1; touched[g1] = 1;
    int a = g0, b = g1;
    // bound: a round either ends the lane or replaces max(a, b) by a strictly smaller id (the value the lost compare-and-swap returned; track_find only
    // lowers further), so a + b falls every round: at most g0 + g1 rounds.  The lane never waits: a lost hook is answered by going on with the pair it saw
    for (;;) {
        a = track_find(parent, a); b = track_find(parent, b);
        if (a == b) break;                                         // a common ancestor: one component already
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(parent + hi, hi, lo);            // hooks hi only while it is a root
        if (old >= hi) break;                                      // old == hi: hooked
        a = old; b = lo;
    }
}

static __global__ void __launch_bounds__(kTrackBlock)
k_tracks_roots(int total, const int* __restrict__ parent, const int* __restrict__ touched, int* __restrict__ root, int* __restrict__ flag, int* __restrict__ sums) {
    const int g = blockIdx.x * kTrackBlock + threadIdx.x;
    int f = 0;
    if (g < total) {
        int r = g;
        // bound: r strictly falls and ids are >= 0: at most g steps
        for (;;) { const int p = parent[r]; if (p >= r) break; r = p; }
        root[g] = r;
        f = (touched[g] != 0) & (r == g);
        flag[g] = f;
    }
    int all; (void)block_exclusive_scan(f, &all);
    if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

// sums[0 .. nb): exclusive scan in place (one workgroup); *grand = the total
static __global__ void __launch_bounds__(kTrackBlock)
k_tracks_scan_sums(int nb, int* __restrict__ sums, int* __restrict__ grand) {
    int carry = 0;
    for (int b = 0; b < nb; b += kTrackBlock) {                    // bound: nb / 256 rounds
        const int i = b + threadIdx.x, v = i < nb ? sums[i] : 0;
        int all; const int ex = block_exclusive_scan(v, &all);
        if (i < nb) sums[i] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) *grand = carry;
}

static __global__ void __launch_bounds__(kTrackBlock)
k_tracks_ids(int total, const int* __restrict__ flag, const int* __restrict__ sums, int* __restrict__ id) {
    const int g = blockIdx.x * kTrackBlock + threadIdx.x;
    const int f = g < total ? flag[g] : 0;
    int all; const int ex = block_exclusive_scan(f, &all);
    if (f) id[g] = sums[blockIdx.x] + ex;
}

static __global__ void __launch_bounds__(kTrackBlock)
k_tracks_assign(int total, int num_frames, const int* __restrict__ feat_ptr, const int* __restrict__ touched, const int* __restrict__ root,
                const int* __restrict__ id, int* __restrict__ tracks, unsigned long long* __restrict__ keys, int* __restrict__ vals, unsigned long long table_mask,
                unsigned* __restrict__ slot) {
    const int g = blockIdx.x * kTrackBlock + threadIdx.x;
    if (g >= total) return;
    if (!touched[g]) { tracks[g] = -1; return; }
    const int t = id[root[g]];
    tracks[g] = t;
    const unsigned long long key = ((unsigned long long)(unsigned)track_segment(feat_ptr, num_frames, g) << 32) | (unsigned long long)(unsigned)t;
    unsigned long long h = ((key * 0x9E3779B97F4A7C15ull) >> 24) & table_mask;
    // bound: the table has table_mask + 1 >= 2 * total slots and at most `total` keys are ever stored, so a free slot or the key's own is met within
    // table_mask + 1 probes; the count bounds the loop by itself.  A slot taken by another key is passed, never waited for
    for (unsigned long long probe = 0; probe <= table_mask; probe++) {
        const unsigned long long old = atomicCAS(keys + h, kTrackEmptyKey, key);
        if (old == kTrackEmptyKey || old == key) { atomicMin(vals + h, g); slot[g] = (unsigned)h; return; }
        h = (h + 1) & table_mask;
    }
    slot[g] = 0u;                                                  // not reached (the bound above); keeps k_tracks_winners inside the table all the same
}

static __global__ void __launch_bounds__(kTrackBlock)
k_tracks_winners(int total, const int* __restrict__ touched, const int* __restrict__ tracks, const int* __restrict__ vals, const unsigned* __restrict__ slot,
                 int* __restrict__ win, unsigned char* __restrict__ conflict, int* __restrict__ sums) {
    const int g = blockIdx.x * kTrackBlock + threadIdx.x;
    int w = 0;
    if (g < total) {
        if (touched[g]) {
            w = vals[slot[g]] == g;
            if (!w && (unsigned)tracks[g] < (unsigned)total) conflict[tracks[g]] = 1;                    // a second feature of this camera on the track (every writer stores the same value)
        }
        win[g] = w;
    }
    int all; (void)block_exclusive_scan(w, &all);
    if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

static __global__ void __launch_bounds__(kTrackBlock)
k_tracks_compact(int total, const int* __restrict__ win, const int* __restrict__ sums, const int* __restrict__ tracks, int* __restrict__ obs_g, int* __restrict__ obs_pt) {
    const int g = blockIdx.x * kTrackBlock + threadIdx.x;
    const int w = g < total ? win[g] : 0;
    int all; const int ex = block_exclusive_scan(w, &all);
    if (w) { const int o = sums[blockIdx.x] + ex; obs_g[o] = g; obs_pt[o] = tracks[g]; }      // o < number of winners <= total
}

namespace {

inline size_t track_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// the context's grow-only scratch of this call (ssfm_ctx.h): one device block, one pinned block
int tracks_reserve(ssfm_ctx* ctx, size_t dev_bytes, size_t pin_bytes) {
    if (ctx->tracks_dev_bytes < dev_bytes) {
        if (ctx->tracks_dev) (void)hipFree(ctx->tracks_dev);
        ctx->tracks_dev = nullptr; ctx->tracks_dev_bytes = 0;
        SSFM_HIP_CHECK(ctx, hipMalloc(&ctx->tracks_dev, dev_bytes));
        ctx->tracks_dev_bytes = dev_bytes;
    }
    if (ctx->tracks_pin_bytes < pin_bytes) {
        if (ctx->tracks_pin) (void)hipHostFree(ctx->tracks_pin);
        ctx->tracks_pin = nullptr; ctx->tracks_pin_bytes = 0;
        SSFM_HIP_CHECK(ctx, hipHostMalloc(&ctx->tracks_pin, pin_bytes, hipHostMallocDefault));
        ctx->tracks_pin_bytes = pin_bytes;
    }
    return SSFM_OK;
}

}  // namespace
}  // namespace ssfm

using namespace ssfm;

extern "C" int ssfm_tracks_last_kernel_ms(ssfm_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SSFM_ERR_INVALID;
    *ms = ctx->tracks_kernel_ms;
    return SSFM_OK;
}

extern "C" int ssfm_build_tracks_device(ssfm_ctx* ctx, int32_t num_keyframes, const int32_t* feat_ptr, const double* feat_xy, int32_t num_match_sets,
                                        const int32_t* ms_index0, const int32_t* ms_index1, const int32_t* ms_ptr, const int32_t* m_f0, const int32_t* m_f1,
                                        double centerx, double centery, int32_t* tracks, int32_t* num_points, uint8_t* point_conflict, int64_t* num_observations,
                                        int32_t* obs_cam, int32_t* obs_pt, int32_t* obs_feat, double* obs_xy) {
    const std::string who = "ssfm_build_tracks_device";
    // the argument checks come before anything touches a device, and before the context is looked at
    if (!feat_ptr || !tracks || !num_points || !num_observations) return fail(ctx, SSFM_ERR_INVALID, who + ": feat_ptr, tracks, num_points and num_observations are required");
    const bool want_obs = obs_cam || obs_pt || obs_feat || obs_xy;
    if (want_obs && !(obs_cam && obs_pt && obs_feat && obs_xy)) return fail(ctx, SSFM_ERR_INVALID, who + ": obs_cam, obs_pt, obs_feat and obs_xy are given together or not at all");
    if (num_match_sets < 0 || (num_match_sets > 0 && (!ms_index0 || !ms_index1 || !ms_ptr))) return fail(ctx, SSFM_ERR_INVALID, who + ": ms_index0, ms_index1 and ms_ptr are required, num_match_sets is >= 0");
    if (num_keyframes <= 0) return fail(ctx, SSFM_ERR_INVALID, who + ": num_keyframes must be positive");
    if (feat_ptr[0] != 0) return fail(ctx, SSFM_ERR_INVALID, who + ": feat_ptr[0] must be 0");
    for (int32_t k = 0; k < num_keyframes; k++) if (feat_ptr[k + 1] < feat_ptr[k]) return fail(ctx, SSFM_ERR_INVALID, who + ": feat_ptr must ascend");
    const int32_t total = feat_ptr[num_keyframes];
    if (total > (1 << 30)) return fail(ctx, SSFM_ERR_INVALID, who + ": more than 2^30 features");
    if (want_obs && total > 0 && !feat_xy) return fail(ctx, SSFM_ERR_INVALID, who + ": feat_xy is null");
    if (num_match_sets > 0 && ms_ptr[0] != 0) return fail(ctx, SSFM_ERR_INVALID, who + ": ms_ptr[0] must be 0");
    for (int32_t s = 0; s < num_match_sets; s++) if (ms_ptr[s + 1] < ms_ptr[s]) return fail(ctx, SSFM_ERR_INVALID, who + ": ms_ptr must ascend");
    const int32_t M = num_match_sets > 0 ? ms_ptr[num_match_sets] : 0;
    if (M > 0 && (!m_f0 || !m_f1)) return fail(ctx, SSFM_ERR_INVALID, who + ": m_f0 and m_f1 are required");
    for (int32_t s = 0; s < num_match_sets; s++)
        if (ms_index0[s] < 0 || ms_index0[s] >= num_keyframes || ms_index1[s] < 0 || ms_index1[s] >= num_keyframes) return fail(ctx, SSFM_ERR_INVALID, who + ": frame index out of range");
    if (!ctx) return fail(nullptr, SSFM_ERR_INVALID, who + ": ctx is null");
    if (ctx->collective) return fail(ctx, SSFM_ERR_INVALID, who + ": the context carries a communicator; this call is single-GPU");

    ctx->tracks_kernel_ms = 0.0;
    *num_points = 0; *num_observations = 0;
    if (M == 0 || total == 0) {                                     // no match names a feature (a match into an empty frame is caught below when total > 0)
        if (M > 0) return fail(ctx, SSFM_ERR_INVALID, who + ": feature index out of range");
        for (int32_t g = 0; g < total; g++) tracks[g] = -1;
        return SSFM_OK;
    }
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t T = (size_t)total, S = (size_t)num_match_sets, K = (size_t)num_keyframes, Mz = (size_t)M;
    const int nb = (int)((T + kTrackBlock - 1) / kTrackBlock);
    size_t table = 1024; while (table < 2 * T) table <<= 1;        // at least twice the features that can be touched

    // ---- layout of the device block and of the pinned block (payload: the uploads, then, once they have been consumed, the downloads)
    size_t d = 0;
    auto carve = [&](size_t bytes) { const size_t at = d; d += track_align(bytes); return at; };
    const size_t o_cnt = carve(4 * sizeof(int)), o_fptr = carve((K + 1) * 4), o_sets = carve(S * sizeof(TrackSet)), o_msptr = carve((S + 1) * 4), o_f0 = carve(Mz * 4), o_f1 = carve(Mz * 4);
    const size_t o_parent = carve(T * 4), o_touched = carve(T * 4), o_root = carve(T * 4), o_flag = carve(T * 4), o_id = carve(T * 4), o_tracks = carve(T * 4), o_slot = carve(T * 4);
    const size_t o_win = carve(T * 4), o_sums = carve((size_t)nb * 4), o_keys = carve(table * 8), o_vals = carve(table * 4), o_conf = carve(T), o_obsg = carve(T * 4), o_obsp = carve(T * 4);
    const size_t dev_bytes = d;
    const size_t u_fptr = 0, u_sets = u_fptr + track_align((K + 1) * 4), u_msptr = u_sets + track_align(S * sizeof(TrackSet)), u_f0 = u_msptr + track_align((S + 1) * 4),
                 u_f1 = u_f0 + track_align(Mz * 4), up_bytes = u_f1 + track_align(Mz * 4);
    const size_t w_tracks = 0, w_conf = w_tracks + track_align(T * 4), w_obsg = w_conf + track_align(T), w_obsp = w_obsg + track_align(T * 4), down_bytes = w_obsp + track_align(T * 4);
    const size_t pin_head = 256;                                    // the counters
    { const int r = tracks_reserve(ctx, dev_bytes, pin_head + std::max(up_bytes, down_bytes)); if (r) return r; }
    char* D = (char*)ctx->tracks_dev; char* H = (char*)ctx->tracks_pin + pin_head; int* h_cnt = (int*)ctx->tracks_pin;
    int* d_cnt = (int*)(D + o_cnt); int* d_fptr = (int*)(D + o_fptr); TrackSet* d_sets = (TrackSet*)(D + o_sets); int* d_msptr = (int*)(D + o_msptr);
    int* d_f0 = (int*)(D + o_f0); int* d_f1 = (int*)(D + o_f1); int* d_parent = (int*)(D + o_parent); int* d_touched = (int*)(D + o_touched); int* d_root = (int*)(D + o_root);
    int* d_flag = (int*)(D + o_flag); int* d_id = (int*)(D + o_id); int* d_tracks = (int*)(D + o_tracks); unsigned* d_slot = (unsigned*)(D + o_slot); int* d_win = (int*)(D + o_win);
    int* d_sums = (int*)(D + o_sums); unsigned long long* d_keys = (unsigned long long*)(D + o_keys); int* d_vals = (int*)(D + o_vals); unsigned char* d_conf = (unsigned char*)(D + o_conf);
    int* d_obsg = (int*)(D + o_obsg); int* d_obsp = (int*)(D + o_obsp);

    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto body = [&]() -> int {
        // ---- uploads through the pinned block; the copy of m_f1 into it overlaps the transfer of m_f0
        std::memcpy(H + u_fptr, feat_ptr, (K + 1) * 4);
        TrackSet* hs = (TrackSet*)(H + u_sets);
        for (size_t s = 0; s < S; s++) { const int a = ms_index0[s], b = ms_index1[s]; hs[s] = TrackSet{feat_ptr[a], feat_ptr[a + 1] - feat_ptr[a], feat_ptr[b], feat_ptr[b + 1] - feat_ptr[b]}; }
        std::memcpy(H + u_msptr, ms_ptr, (S + 1) * 4);
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(d_fptr, H + u_fptr, (K + 1) * 4, hipMemcpyHostToDevice, st));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(d_sets, H + u_sets, S * sizeof(TrackSet), hipMemcpyHostToDevice, st));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(d_msptr, H + u_msptr, (S + 1) * 4, hipMemcpyHostToDevice, st));
        std::memcpy(H + u_f0, m_f0, Mz * 4);
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(d_f0, H + u_f0, Mz * 4, hipMemcpyHostToDevice, st));
        std::memcpy(H + u_f1, m_f1, Mz * 4);
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(d_f1, H + u_f1, Mz * 4, hipMemcpyHostToDevice, st));
        SSFM_HIP_CHECK(ctx, hipEventCreate(&e0)); SSFM_HIP_CHECK(ctx, hipEventCreate(&e1));
        SSFM_HIP_CHECK(ctx, hipEventRecord(e0, st));
        SSFM_HIP_CHECK(ctx, hipMemsetAsync(d_cnt, 0, 4 * sizeof(int), st));
        SSFM_HIP_CHECK(ctx, hipMemsetAsync(d_keys, 0xFF, table * 8, st));              // kTrackEmptyKey
        SSFM_HIP_CHECK(ctx, hipMemsetAsync(d_vals, 0x7F, table * 4, st));              // 0x7F7F7F7F: above every feature id (total <= 2^30)
        SSFM_HIP_CHECK(ctx, hipMemsetAsync(d_conf, 0, T, st));
        const dim3 gt((unsigned)nb), gm((unsigned)((Mz + kTrackBlock - 1) / kTrackBlock)), blk(kTrackBlock);
        hipLaunchKernelGGL(k_tracks_init, gt, blk, 0, st, total, d_parent, d_touched);
        hipLaunchKernelGGL(k_tracks_link, gm, blk, 0, st, M, num_match_sets, d_msptr, d_sets, d_f0, d_f1, d_parent, d_touched, d_cnt + 2);
        hipLaunchKernelGGL(k_tracks_roots, gt, blk, 0, st, total, d_parent, d_touched, d_root, d_flag, d_sums);
        hipLaunchKernelGGL(k_tracks_scan_sums, dim3(1), blk, 0, st, nb, d_sums, d_cnt + 0);
        hipLaunchKernelGGL(k_tracks_ids, gt, blk, 0, st, total, d_flag, d_sums, d_id);
        hipLaunchKernelGGL(k_tracks_assign, gt, blk, 0, st, total, num_keyframes, d_fptr, d_touched, d_root, d_id, d_tracks, d_keys, d_vals, (unsigned long long)(table - 1), d_slot);
        hipLaunchKernelGGL(k_tracks_winners, gt, blk, 0, st, total, d_touched, d_tracks, d_vals, d_slot, d_win, d_conf, d_sums);
        hipLaunchKernelGGL(k_tracks_scan_sums, dim3(1), blk, 0, st, nb, d_sums, d_cnt + 1);
        hipLaunchKernelGGL(k_tracks_compact, gt, blk, 0, st, total, d_win, d_sums, d_tracks, d_obsg, d_obsp);
        SSFM_HIP_CHECK(ctx, hipGetLastError());
        SSFM_HIP_CHECK(ctx, hipEventRecord(e1, st));
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(h_cnt, d_cnt, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        { float ms = 0.f; if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ctx->tracks_kernel_ms = ms; else (void)hipGetLastError(); }
        if (h_cnt[2]) return fail(ctx, SSFM_ERR_INVALID, who + ": feature index out of range");
        const size_t P = (size_t)std::min(std::max(h_cnt[0], 0), total), N = (size_t)std::min(std::max(h_cnt[1], 0), total);
        // ---- downloads (the uploads have been consumed: the payload area is free)
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(H + w_tracks, d_tracks, T * 4, hipMemcpyDeviceToHost, st));
        if (point_conflict && P) SSFM_HIP_CHECK(ctx, hipMemcpyAsync(H + w_conf, d_conf, P, hipMemcpyDeviceToHost, st));
        if (want_obs && N) {
            SSFM_HIP_CHECK(ctx, hipMemcpyAsync(H + w_obsg, d_obsg, N * 4, hipMemcpyDeviceToHost, st));
            SSFM_HIP_CHECK(ctx, hipMemcpyAsync(H + w_obsp, d_obsp, N * 4, hipMemcpyDeviceToHost, st));
        }
        SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        std::memcpy(tracks, H + w_tracks, T * 4);
        if (point_conflict && P) std::memcpy(point_conflict, H + w_conf, P);
        if (want_obs && N) {
            const int* hg = (const int*)(H + w_obsg);
            std::memcpy(obs_pt, H + w_obsp, N * 4);
            int cam = 0;
            for (size_t o = 0; o < N; o++) {                        // g ascends: the camera only moves forward
                const int g = hg[o];
                if (g < 0 || g >= total) return fail(ctx, SSFM_ERR_HIP, who + ": the device returned a feature id out of range");
                while (feat_ptr[cam + 1] <= g) cam++;               // bound: g < feat_ptr[num_keyframes]
                obs_cam[o] = cam; obs_feat[o] = g - feat_ptr[cam];
                obs_xy[2 * o] = feat_xy[2 * (size_t)g] - centerx; obs_xy[2 * o + 1] = feat_xy[2 * (size_t)g + 1] - centery;
            }
        }
        *num_points = (int32_t)P; *num_observations = (int64_t)N;
        return SSFM_OK;
    };
    const int rc = body();
    if (rc != SSFM_OK) (void)hipStreamSynchronize(st);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}
