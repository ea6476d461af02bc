// spherical_sfm_amd -- host side of ssfm_anms_batch (include/ssfm.h): the argument checks, the work list of the radius kernel with its j split, and a plain host
// implementation of the contract (ssfm_anms_batch_host; the check of tests/native/anms_host_check.cpp and the CPU side of scripts/anms_timing.py).
// Plain C++ without a device: anms.hip includes it, and so does tests/native/anms_host_check.cpp, which runs it under ASan + UBSan.
#pragma once
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <thread>
#include <vector>
#include "../../include/ssfm.h"

namespace ssfm {

constexpr int32_t kAnmsBlock = 256;         // lanes of a radius workgroup = keypoints i of one work item
constexpr int32_t kAnmsTile = 1024;         // keypoints j of one LDS tile (16 B each)
constexpr int32_t kAnmsMinChunk = 256;      // the planner cuts no j chunk shorter than this

// nullptr when the call may go on, otherwise the reason it is refused (SSFM_ERR_INVALID).  Arguments first, then kp_ptr, num_to_keep and the responses; the
// context is looked at after all of them.
inline const char* anms_check(int32_t num_frames, const int32_t* kp_ptr, const float* xy, const float* response, const int32_t* num_to_keep,
                              const ssfm_anms_options* o, const int32_t* keep_ptr, const int32_t* keep_idx) {
    if (num_frames < 0 || !kp_ptr || !keep_ptr || (num_frames > 0 && !num_to_keep)) return "bad arguments";
    if (o && o->force_j_chunks < 0) return "bad options";
    if (kp_ptr[0] != 0) return "kp_ptr does not start at 0";
    for (int32_t f = 0; f < num_frames; f++)
        if (kp_ptr[f + 1] < kp_ptr[f]) return "kp_ptr is not ascending";
    const int32_t total = kp_ptr[num_frames];
    if (total > (1 << 30) /* i0 + 256 and the byte offsets of xy stay in range */ || (total > 0 && (!xy || !response || !keep_idx))) return "bad arguments";
    for (int32_t f = 0; f < num_frames; f++)
        if (num_to_keep[f] < 0) return "num_to_keep is negative";
    for (int32_t k = 0; k < total; k++)
        if (response[k] != response[k]) return "NaN response";
    return nullptr;
}

// One workgroup of the radius kernel: the keypoints i0 .. i0 + kAnmsBlock of the frame at kp0 (n keypoints) against its keypoints j_lo .. j_hi.
// split: the frame's j range is cut, the item combines its minimum and its count with atomics; otherwise it owns its i and stores.
struct AnmsItem { int32_t kp0, n, i0, j_lo, j_hi, split; };

// A frame takes part in the radius kernel when it has keypoints and is not returned unchanged (n < num_to_keep).
inline bool anms_frame_active(int32_t n, int32_t keep) { return n > 0 && n >= keep; }

// The j chunk length of a frame.  force > 0: that many chunks (fewer when n is smaller), of ceil(n / force) each.  Otherwise the call's `want` chunks
// (anms_plan), in multiples of 64 and no shorter than kAnmsMinChunk.
inline int32_t anms_chunk_len(int32_t n, int32_t want, int32_t force) {
    if (force > 0) return std::max<int32_t>(1, (int32_t)(((int64_t)n + force - 1) / force));
    if (want <= 1) return n;
    const int64_t len = ((((int64_t)n + want - 1) / want + 63) / 64) * 64;
    return (int32_t)std::min<int64_t>(n, std::max<int64_t>(len, kAnmsMinChunk));
}

// The work list.  Frames that together fill the device (8 workgroups per compute unit: a workgroup is one wave on each SIMD, and eight waves fit one) are not
// cut; below that every frame is cut into as many chunks as make up the difference.  Returns the number of items that combine with atomics.
inline int64_t anms_plan(int32_t num_frames, const int32_t* kp_ptr, const int32_t* num_to_keep, int32_t force, int32_t num_cus, std::vector<AnmsItem>& items) {
    items.clear();
    int64_t blocks = 0;
    for (int32_t f = 0; f < num_frames; f++) {
        const int32_t n = kp_ptr[f + 1] - kp_ptr[f];
        if (anms_frame_active(n, num_to_keep[f])) blocks += (n + kAnmsBlock - 1) / kAnmsBlock;
    }
    const int64_t target = 8 * (int64_t)std::max(num_cus, 1);
    const int32_t want = (blocks > 0 && blocks < target) ? (int32_t)((target + blocks - 1) / blocks) : 1;
    int64_t split_items = 0;
    for (int32_t f = 0; f < num_frames; f++) {
        const int32_t n = kp_ptr[f + 1] - kp_ptr[f];
        if (!anms_frame_active(n, num_to_keep[f])) continue;
        const int32_t len = anms_chunk_len(n, want, force), chunks = (int32_t)(((int64_t)n + len - 1) / len);
        for (int32_t i0 = 0; i0 < n; i0 += kAnmsBlock)
            for (int32_t c = 0; c < chunks; c++) {
                items.push_back(AnmsItem{kp_ptr[f], n, i0, c * len, (int32_t)std::min<int64_t>(n, (int64_t)(c + 1) * len), chunks > 1 ? 1 : 0});
                split_items += chunks > 1;
            }
    }
    return split_items;
}

// ---- the contract on the host ----------------------------------------------------------------------------------------------------------
// The total order (response descending, original index ascending) is what a stable sort by response gives; in it the j with response_j > thr_i form a
// prefix of the positions before i, which is the reference's loop with its early exit.

inline void anms_sorted_order(int32_t n, const float* response, int32_t* order) {
    std::iota(order, order + n, 0);
    std::stable_sort(order, order + n, [&](int32_t a, int32_t b) { return response[a] > response[b]; });
}

// radius of the keypoints at the sorted positions p_lo .. p_hi, written per INPUT keypoint.  sx, sy, sr: the frame's keypoints in sorted order.  The responses
// descend, so the reference's loop condition `j < i && response_j > thr` holds on a prefix whose end a binary search finds; the loop over it has no exit.
inline void anms_radii_host(const float* sx, const float* sy, const float* sr, const int32_t* order, int32_t p_lo, int32_t p_hi, double* radius) {
    for (int32_t p = p_lo; p < p_hi; p++) {
        const float thr = sr[p] * 1.11f, xi = sx[p], yi = sy[p];
        const int32_t m = (int32_t)(std::partition_point(sr, sr + p, [thr](float v) { return v > thr; }) - sr);
        double acc[4] = {INFINITY, INFINITY, INFINITY, INFINITY};          // four running minima: a minimum does not depend on the order it is taken in
        for (int32_t q = 0; q < m; q++) {
            const float dx = xi - sx[q], dy = yi - sy[q];
            const double d = (double)dx * dx + (double)dy * dy;
            acc[q & 3] = d < acc[q & 3] ? d : acc[q & 3];
        }
        double d2 = INFINITY;
        for (int k = 0; k < 4; k++) d2 = acc[k] < d2 ? acc[k] : d2;
        radius[order[p]] = d2 < INFINITY ? std::sqrt(d2) : DBL_MAX;
    }
}

// the keep list from the radii: element `keep` of the radii sorted descending decides (n == keep: everything); returns the number kept
inline int32_t anms_select_host(int32_t n, int32_t keep, const int32_t* order, const double* radius, int32_t* keep_idx) {
    double decision = 0.0;
    if (keep < n) {
        std::vector<double> r(radius, radius + n);
        std::nth_element(r.begin(), r.begin() + keep, r.end(), [](double a, double b) { return a > b; });
        decision = r[(size_t)keep];
    }
    int32_t m = 0;
    for (int32_t p = 0; p < n; p++)
        if (radius[order[p]] >= decision) keep_idx[m++] = order[p];
    return m;
}

// ssfm_anms_batch on the host (arguments already checked).  Threads share the frames and, within a frame, blocks of sorted positions.
inline void anms_batch_host(int32_t num_frames, const int32_t* kp_ptr, const float* xy, const float* response, const int32_t* num_to_keep, int32_t num_threads,
                            int32_t* keep_ptr, int32_t* keep_idx, double* radius) {
    const int32_t total = kp_ptr[num_frames];
    std::vector<int32_t> order((size_t)total), kept((size_t)total), count((size_t)num_frames, 0);
    std::vector<float> sx((size_t)total), sy((size_t)total), sr((size_t)total);                     // the keypoints in sorted order, frame by frame
    std::vector<double> rad_own;
    if (!radius) { rad_own.resize((size_t)total); radius = rad_own.data(); }
    struct Task { int32_t f, p_lo, p_hi; };
    std::vector<Task> tasks;
    const int32_t kBlock = 512;
    for (int32_t f = 0; f < num_frames; f++) {
        const int32_t n = kp_ptr[f + 1] - kp_ptr[f];
        if (anms_frame_active(n, num_to_keep[f]))
            for (int32_t p = 0; p < n; p += kBlock) tasks.push_back(Task{f, p, std::min(n, p + kBlock)});
    }
    auto run = [&](size_t count_, auto&& body) {
        std::atomic<size_t> next{0};
        auto worker = [&]() { for (size_t k = next++; k < count_; k = next++) body(k); };
        const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(num_threads, 1), count_));
        std::vector<std::thread> th;
        for (int t = 1; t < nt; t++) th.emplace_back(worker);
        worker();
        for (auto& t : th) t.join();
    };
    run((size_t)num_frames, [&](size_t f) {
        const int32_t s = kp_ptr[f], n = kp_ptr[f + 1] - s;
        if (!anms_frame_active(n, num_to_keep[f])) return;
        anms_sorted_order(n, response + s, order.data() + s);
        for (int32_t p = 0; p < n; p++) {
            const size_t g = (size_t)s + (size_t)order[(size_t)s + p];
            sx[(size_t)s + p] = xy[2 * g]; sy[(size_t)s + p] = xy[2 * g + 1]; sr[(size_t)s + p] = response[g];
        }
    });
    run(tasks.size(), [&](size_t k) {
        const int32_t s = kp_ptr[tasks[k].f];
        anms_radii_host(sx.data() + s, sy.data() + s, sr.data() + s, order.data() + s, tasks[k].p_lo, tasks[k].p_hi, radius + s);
    });
    run((size_t)num_frames, [&](size_t f) {
        const int32_t s = kp_ptr[f], n = kp_ptr[f + 1] - s;
        if (anms_frame_active(n, num_to_keep[f])) count[f] = anms_select_host(n, num_to_keep[f], order.data() + s, radius + s, kept.data() + s);
        else { for (int32_t i = 0; i < n; i++) { kept[(size_t)s + i] = i; radius[(size_t)s + i] = DBL_MAX; } count[f] = n; }
    });
    keep_ptr[0] = 0;
    for (int32_t f = 0; f < num_frames; f++) {
        std::copy(kept.begin() + kp_ptr[f], kept.begin() + kp_ptr[f] + count[(size_t)f], keep_idx + keep_ptr[f]);
        keep_ptr[f + 1] = keep_ptr[f] + count[(size_t)f];
    }
}

}  // namespace ssfm
