// spherical_sfm_amd -- the pairwise front end in one call: match_exhaustive + estimate_pairwise (reference examples/spherical_sfm_tools.cpp:575-600 and
// :309-420) or + estimate_pairwise_five_point (:433-573) for a caller-given pair list, with the match lists staying on the device between the two stages.
//
// ssfm_pairwise_from_features is DEFINED as the composition
//   ssfm_match_pairs -> candidates (count >= min_num_inliers, count > 0) -> ssfm_ransac_batch_indexed on the candidates -> num_inliers > min_num_inliers
// and ssfm_pairwise5_from_features as the same with ssfm_ransac5_batch_indexed in the third place.  Both run exactly those kernels with those launch
// parameters (match.hip: match_slabs, ransac.hip: ransac_on_device_lists -- the slab plan is made from the same counts).  What is new here is the hand-over
// around them:
//   k_front_gather    k_gather_rays' job from the device-resident lists of the candidate pairs (every list index is range-checked before it addresses a ray)
//   k_front_count     per candidate: inliers in its mask, acceptance flag
//   k_front_scan      exclusive scans over the slab's pairs (one workgroup): position among the accepted pairs, start of the inlier list
//   k_front_compact   (idx0, idx1) of the inliers of accepted pairs, in list order (= ascending train index); R (column-major) and counts per accepted pair;
//                     the five-point instantiation also t and E (column-major) per accepted pair
// Per pair 4 bytes of counts come back after matching and 8 bytes of diagnostics after RANSAC; the lists and the byte mask never leave the device, only the
// accepted pairs' R / counts / inlier lists do (five-point: + 24 bytes of t, + 72 bytes of E when it is asked for).  No atomics, no inter-workgroup
// waiting: the same bits every run.
#include <algorithm>
#include <cstring>
#include <limits>
#include <vector>
#include "ransac_device.h"
#include "pairwise_front.h"

namespace ssfm {

struct FrontPair { int off0, off1, n0, n1, src; };         // feature offsets / counts of the two frames; where the pair's list starts in the call's lists

static __global__ void __launch_bounds__(256)
k_front_gather(const int* __restrict__ ptr, const FrontPair* __restrict__ info, const int* __restrict__ idx0, const int* __restrict__ idx1, int list_len,
               const double* __restrict__ rays, double* __restrict__ u, double* __restrict__ v, int* __restrict__ bad) {
    const int p = blockIdx.x, a = ptr[p], b = ptr[p + 1];
    const FrontPair I = info[p];
    for (int i = a + threadIdx.x; i < b; i += 256) {
        const long long s = (long long)I.src + (i - a);
        bool ok = s >= 0 && s < (long long)list_len;
        const int i0 = ok ? idx0[s] : -1, i1 = ok ? idx1[s] : -1;
        ok = ok && (unsigned)i0 < (unsigned)I.n0 && (unsigned)i1 < (unsigned)I.n1;
        double r0[3] = {0.0, 0.0, 0.0}, r1[3] = {0.0, 0.0, 0.0};
        if (ok) {
            const double* q0 = rays + 3 * ((size_t)I.off0 + (size_t)i0); const double* q1 = rays + 3 * ((size_t)I.off1 + (size_t)i1);
            r0[0] = q0[0]; r0[1] = q0[1]; r0[2] = q0[2]; r1[0] = q1[0]; r1[1] = q1[1]; r1[2] = q1[2];
        } else *bad = 1;                                             // (every writer stores the same value)
        u[3 * (size_t)i] = r0[0]; u[3 * (size_t)i + 1] = r0[1]; u[3 * (size_t)i + 2] = r0[2];
        v[3 * (size_t)i] = r1[0]; v[3 * (size_t)i + 1] = r1[1]; v[3 * (size_t)i + 2] = r1[2];
    }
}

static __global__ void __launch_bounds__(256)
k_front_count(const int* __restrict__ ptr, const unsigned char* __restrict__ mask, const int* __restrict__ nin, int min_num_inliers, int* __restrict__ cnt,
              int* __restrict__ acc) {
    const int p = blockIdx.x, a = ptr[p], b = ptr[p + 1];
    int c = 0;
    for (int i = a + threadIdx.x; i < b; i += 256) c += mask[i] != 0;
    int total; (void)block_exclusive_scan(c, &total);
    if (threadIdx.x == 0) {
        const int ok = nin[p] > min_num_inliers && total > 0;        // spherical_sfm_tools.cpp:410, and a non-empty inlier list
        acc[p] = ok; cnt[p] = ok ? total : 0;
    }
}

// apos[0 .. np] / optr[0 .. np]: exclusive scans of acc / cnt (one workgroup); tot = {accepted pairs, inlier matches}
static __global__ void __launch_bounds__(256)
k_front_scan(int np, const int* __restrict__ cnt, const int* __restrict__ acc, int* __restrict__ optr, int* __restrict__ apos, int* __restrict__ tot) {
    int carry_c = 0, carry_a = 0;
    for (int b = 0; b < np; b += 256) {
        const int i = b + threadIdx.x, c = i < np ? cnt[i] : 0, a = i < np ? acc[i] : 0;
        int tc, ta; const int ec = block_exclusive_scan(c, &tc); const int ea = block_exclusive_scan(a, &ta);
        if (i < np) { optr[i] = carry_c + ec; apos[i] = carry_a + ea; }
        carry_c += tc; carry_a += ta;
    }
    if (threadIdx.x == 0) { optr[np] = carry_c; apos[np] = carry_a; tot[0] = carry_a; tot[1] = carry_c; }
}

// meta[3 a] = {slab-local pair, num_inliers, start of the inlier list} of accepted pair a; Racc[9 a]: its rotation, column-major
// FIVE: also Eacc[9 a], its essential matrix, column-major, and Tacc[3 a], its translation (one wave each for R, E and t: three independent loads)
template <bool FIVE> static __global__ void __launch_bounds__(256)
k_front_compact(const int* __restrict__ ptr, const unsigned char* __restrict__ mask, const FrontPair* __restrict__ info, const int* __restrict__ idx0,
                const int* __restrict__ idx1, int list_len, const int* __restrict__ optr, const int* __restrict__ apos, const int* __restrict__ acc,
                const int* __restrict__ nin, const double* __restrict__ R, const double* __restrict__ E, const double* __restrict__ T, int out_cap,
                int* __restrict__ o0, int* __restrict__ o1, double* __restrict__ Racc, double* __restrict__ Eacc, double* __restrict__ Tacc, int* __restrict__ meta) {
    const int p = blockIdx.x;
    if (!acc[p]) return;                                             // (uniform over the workgroup)
    const int r0 = ptr[p], n = ptr[p + 1] - r0, a = apos[p], src = info[p].src;
    int base = optr[p];
    if (threadIdx.x < 9) Racc[9 * (size_t)a + (threadIdx.x / 3) + 3 * (threadIdx.x % 3)] = R[9 * (size_t)p + threadIdx.x];      // row-major -> column-major
    if constexpr (FIVE) {
        const int q = (int)threadIdx.x - 64, c = (int)threadIdx.x - 128;
        if (q >= 0 && q < 9) Eacc[9 * (size_t)a + (q / 3) + 3 * (q % 3)] = E[9 * (size_t)p + q];
        if (c >= 0 && c < 3) Tacc[3 * (size_t)a + c] = T[3 * (size_t)p + c];
    }
    if (threadIdx.x == 0) { meta[3 * a] = p; meta[3 * a + 1] = nin[p]; meta[3 * a + 2] = base; }
    for (int b = 0; b < n; b += 256) {
        const int i = b + threadIdx.x;
        const long long s = (long long)src + i;
        const bool in = i < n && mask[r0 + i] != 0 && s >= 0 && s < (long long)list_len;
        int total; const int ex = block_exclusive_scan(in, &total);
        if (in && base + ex < out_cap) { o0[base + ex] = idx0[s]; o1[base + ex] = idx1[s]; }
        base += total;
    }
}

namespace {

struct FrontHooks : RansacDeviceLists {
    ssfm_ctx* ctx = nullptr; const char* who = ""; bool five = false;
    // the call's match lists on the device and the candidate table on the host
    const int* d_idx0 = nullptr; const int* d_idx1 = nullptr; int list_len = 0; const double* d_frays = nullptr;
    const int32_t* feat_ptr = nullptr; const int32_t* cf0 = nullptr; const int32_t* cf1 = nullptr; const int32_t* csrc = nullptr; const int32_t* cand = nullptr;
    int min_num_inliers = 0;
    // the caller's outputs
    int64_t pair_capacity = 0, inlier_capacity = 0;
    int32_t* accepted_pair = nullptr; double* R = nullptr; double* t = nullptr; double* E = nullptr; int32_t* num_inliers = nullptr; int32_t* inl_ptr = nullptr; int32_t* inl_idx0 = nullptr; int32_t* inl_idx1 = nullptr;
    int64_t acc_run = 0, inl_run = 0; bool overflow = false;
    struct Slot { DevBuf<FrontPair> info; DevBuf<int> cnt, acc, optr, apos, tot, o0, o1, meta; DevBuf<double> Racc, Eacc, Tacc; FrontPair* h_info = nullptr; int* h_tot = nullptr; } slot[2];
    int cap_pairs = 0; size_t cap_rays = 0;
    std::vector<int> hmeta;

    int prepare(int nslot, int cap_pairs_, size_t cap_rays_) override {
        cap_pairs = cap_pairs_; cap_rays = cap_rays_;
        for (int b = 0; b < nslot; b++) {
            Slot& s = slot[b];
            SSFM_HIP_CHECK(ctx, s.info.alloc(cap_pairs)); SSFM_HIP_CHECK(ctx, s.cnt.alloc(cap_pairs)); SSFM_HIP_CHECK(ctx, s.acc.alloc(cap_pairs));
            SSFM_HIP_CHECK(ctx, s.optr.alloc((size_t)cap_pairs + 1)); SSFM_HIP_CHECK(ctx, s.apos.alloc((size_t)cap_pairs + 1)); SSFM_HIP_CHECK(ctx, s.tot.alloc(3));
            SSFM_HIP_CHECK(ctx, s.o0.alloc(cap_rays)); SSFM_HIP_CHECK(ctx, s.o1.alloc(cap_rays)); SSFM_HIP_CHECK(ctx, s.meta.alloc((size_t)3 * cap_pairs));
            SSFM_HIP_CHECK(ctx, s.Racc.alloc((size_t)9 * cap_pairs));
            if (five) { SSFM_HIP_CHECK(ctx, s.Eacc.alloc((size_t)9 * cap_pairs)); SSFM_HIP_CHECK(ctx, s.Tacc.alloc((size_t)3 * cap_pairs)); }
            SSFM_HIP_CHECK(ctx, hipHostMalloc((void**)&s.h_info, (size_t)cap_pairs * sizeof(FrontPair), hipHostMallocDefault));
            SSFM_HIP_CHECK(ctx, hipHostMalloc((void**)&s.h_tot, 3 * sizeof(int), hipHostMallocDefault));
        }
        hmeta.resize((size_t)3 * cap_pairs);
        return SSFM_OK;
    }
    int stage(hipStream_t up, int b, int p0, int np) override {
        Slot& s = slot[b];
        for (int i = 0; i < np; i++) {
            const int f0 = cf0[p0 + i], f1 = cf1[p0 + i];
            s.h_info[i] = FrontPair{feat_ptr[f0], feat_ptr[f1], feat_ptr[f0 + 1] - feat_ptr[f0], feat_ptr[f1 + 1] - feat_ptr[f1], csrc[p0 + i]};
        }
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(s.info.p, s.h_info, (size_t)np * sizeof(FrontPair), hipMemcpyHostToDevice, up));
        return SSFM_OK;
    }
    int gather(hipStream_t st, int b, int np, const int* d_ptr, double* d_u, double* d_v) override {
        Slot& s = slot[b];
        SSFM_HIP_CHECK(ctx, hipMemsetAsync(s.tot.p, 0, 3 * sizeof(int), st));
        if (np > 0) hipLaunchKernelGGL(k_front_gather, dim3(np), dim3(256), 0, st, d_ptr, s.info.p, d_idx0, d_idx1, list_len, d_frays, d_u, d_v, s.tot.p + 2);
        SSFM_HIP_CHECK(ctx, hipGetLastError());
        return SSFM_OK;
    }
    int lists(hipStream_t st, int b, int np, const int* d_ptr, const unsigned char* d_mask, const int* d_nin, const double* d_R, const double* d_E,
              const double* d_t) override {
        Slot& s = slot[b];
        if (np > 0) {
            hipLaunchKernelGGL(k_front_count, dim3(np), dim3(256), 0, st, d_ptr, d_mask, d_nin, min_num_inliers, s.cnt.p, s.acc.p);
            hipLaunchKernelGGL(k_front_scan, dim3(1), dim3(256), 0, st, np, s.cnt.p, s.acc.p, s.optr.p, s.apos.p, s.tot.p);
            const int out_cap = (int)std::min<size_t>(cap_rays, (size_t)std::numeric_limits<int>::max());
            if (five) hipLaunchKernelGGL(k_front_compact<true>, dim3(np), dim3(256), 0, st, d_ptr, d_mask, s.info.p, d_idx0, d_idx1, list_len, s.optr.p, s.apos.p, s.acc.p, d_nin,
                                         d_R, d_E, d_t, out_cap, s.o0.p, s.o1.p, s.Racc.p, s.Eacc.p, s.Tacc.p, s.meta.p);
            else hipLaunchKernelGGL(k_front_compact<false>, dim3(np), dim3(256), 0, st, d_ptr, d_mask, s.info.p, d_idx0, d_idx1, list_len, s.optr.p, s.apos.p, s.acc.p, d_nin,
                                    d_R, (const double*)nullptr, (const double*)nullptr, out_cap, s.o0.p, s.o1.p, s.Racc.p, (double*)nullptr, (double*)nullptr, s.meta.p);
            SSFM_HIP_CHECK(ctx, hipGetLastError());
        }
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(s.h_tot, s.tot.p, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
        return SSFM_OK;
    }
    int collect(hipStream_t cp, int b, int p0, int np) override {
        Slot& s = slot[b];
        (void)np;
        const int na = s.h_tot[0], ni = s.h_tot[1];
        if (s.h_tot[2]) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": a match index on the device is out of range");
        if (!overflow && acc_run + na <= pair_capacity && inl_run + ni <= inlier_capacity) {
            if (na) {
                SSFM_HIP_CHECK(ctx, hipMemcpyAsync(hmeta.data(), s.meta.p, (size_t)3 * na * sizeof(int), hipMemcpyDeviceToHost, cp));
                SSFM_HIP_CHECK(ctx, hipMemcpyAsync(R + 9 * (size_t)acc_run, s.Racc.p, (size_t)9 * na * sizeof(double), hipMemcpyDeviceToHost, cp));
                if (five) SSFM_HIP_CHECK(ctx, hipMemcpyAsync(t + 3 * (size_t)acc_run, s.Tacc.p, (size_t)3 * na * sizeof(double), hipMemcpyDeviceToHost, cp));
                if (five && E) SSFM_HIP_CHECK(ctx, hipMemcpyAsync(E + 9 * (size_t)acc_run, s.Eacc.p, (size_t)9 * na * sizeof(double), hipMemcpyDeviceToHost, cp));
                if (ni) {
                    SSFM_HIP_CHECK(ctx, hipMemcpyAsync(inl_idx0 + inl_run, s.o0.p, (size_t)ni * sizeof(int), hipMemcpyDeviceToHost, cp));
                    SSFM_HIP_CHECK(ctx, hipMemcpyAsync(inl_idx1 + inl_run, s.o1.p, (size_t)ni * sizeof(int), hipMemcpyDeviceToHost, cp));
                }
                SSFM_HIP_CHECK(ctx, hipStreamSynchronize(cp));
                for (int a = 0; a < na; a++) {
                    accepted_pair[acc_run + a] = cand[p0 + hmeta[3 * (size_t)a]]; num_inliers[acc_run + a] = hmeta[3 * (size_t)a + 1];
                    inl_ptr[acc_run + a] = (int32_t)(inl_run + hmeta[3 * (size_t)a + 2]);
                }
            }
        } else overflow = true;                                      // keep counting: the call reports both sizes
        acc_run += na; inl_run += ni;
        return SSFM_OK;
    }
    void release() {
        for (int b = 0; b < 2; b++) {
            Slot& s = slot[b];
            s.info.free(); s.cnt.free(); s.acc.free(); s.optr.free(); s.apos.free(); s.tot.free(); s.o0.free(); s.o1.free(); s.meta.free(); s.Racc.free(); s.Eacc.free(); s.Tacc.free();
            if (s.h_info) (void)hipHostFree(s.h_info); if (s.h_tot) (void)hipHostFree(s.h_tot);
            s.h_info = nullptr; s.h_tot = nullptr;
        }
    }
};

}  // namespace
}  // namespace ssfm

using namespace ssfm;

extern "C" int ssfm_pairwise_front_last_kernel_ms(ssfm_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SSFM_ERR_INVALID;
    *ms = ctx->front_kernel_ms;
    return SSFM_OK;
}

// both entry points; five: the five-point estimator, t required, E optional (spherical: both null)
static int front_impl(const char* who, bool five, ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, const double* feat_rays, int32_t num_pairs,
                      const int32_t* pair_frame0, const int32_t* pair_frame1, const ssfm_match_options* match_opt, const ssfm_ransac_options* ransac_opt,
                      double squared_inlier_threshold, int64_t pair_capacity, int64_t inlier_capacity, int64_t* needed, int32_t* accepted_pair, double* R, double* t, double* E,
                      int32_t* num_inliers, int32_t* inl_ptr, int32_t* inl_idx0, int32_t* inl_idx1, int32_t* match_count, int32_t* num_inliers_all, uint32_t* stats) {
    // the argument checks come before anything touches a device (and before the context is looked at: without one the message goes to ssfm_last_error(NULL))
    if (!needed || !accepted_pair || !R || (five && !t) || !num_inliers || !inl_ptr || !inl_idx0 || !inl_idx1 || pair_capacity < 0 || inlier_capacity < 0)
        return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": needed, accepted_pair, R, " + (five ? "t, " : "") + "num_inliers, inl_ptr, inl_idx0 and inl_idx1 are required, the capacities are >= 0");
    ssfm_match_options MO; ssfm_match_default_options(&MO);
    if (num_frames == 0 && num_pairs > 0) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": frame index out of range");
    if (num_frames != 0 || num_pairs != 0) {
        const int r = match_check_args(ctx, who, num_frames, feat_ptr, descs, num_pairs, pair_frame0, pair_frame1, match_opt, &MO); if (r) return r;
        if (feat_ptr[num_frames] && !feat_rays) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": feat_rays is null");
    }
    if (!ctx) return fail(nullptr, SSFM_ERR_INVALID, std::string(who) + ": ctx is null");
    if (ctx->collective) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": the context carries a communicator; this call is single-GPU" + (five ? "" : " (multi-GPU: ssfm_match_pairs + ssfm_ransac_batch_indexed_sharded)"));
    ssfm_ransac_options RO; if (ransac_opt) RO = *ransac_opt; else ssfm_ransac_default_options(&RO);
    needed[0] = needed[1] = 0; inl_ptr[0] = 0;
    ctx->front_kernel_ms = 0.0;
    for (int p = 0; p < num_pairs; p++) {
        if (match_count) match_count[p] = 0;
        if (num_inliers_all) num_inliers_all[p] = -1;
        if (stats) stats[2 * (size_t)p] = stats[2 * (size_t)p + 1] = 0;
    }
    if (num_pairs == 0) return SSFM_OK;
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // 1. matching: the compacted lists of every slab are appended to one device-resident list; only the counts come back
    std::vector<int32_t> mp((size_t)num_pairs + 1, 0);
    DevBuf<int> all0, all1, old0, old1; DevBuf<double> frays; size_t cap = 0, used = 0;
    FrontHooks H;
    auto body = [&]() -> int {
        int rc = match_slabs(ctx, num_frames, feat_ptr, descs, num_pairs, pair_frame0, pair_frame1, MO, [&](int p0, int np, const int* hptr, const int* d0, const int* d1) -> int {
            const size_t slab_total = (size_t)hptr[np];
            if (used + slab_total > (size_t)std::numeric_limits<int32_t>::max()) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": more than INT32_MAX matches in one call");
            for (int i = 1; i <= np; i++) mp[(size_t)p0 + i] = (int32_t)(used + (size_t)hptr[i]);
            if (used + slab_total > cap) {                           // grow (the last slab takes exactly what is left)
                const size_t ncap = (p0 + np == num_pairs) ? used + slab_total : std::max(used + slab_total, 2 * cap);
                old0 = all0; old1 = all1; all0 = DevBuf<int>(); all1 = DevBuf<int>();
                SSFM_HIP_CHECK(ctx, all0.alloc(ncap)); SSFM_HIP_CHECK(ctx, all1.alloc(ncap));
                if (used) {
                    SSFM_HIP_CHECK(ctx, hipMemcpyAsync(all0.p, old0.p, used * sizeof(int), hipMemcpyDeviceToDevice, st));
                    SSFM_HIP_CHECK(ctx, hipMemcpyAsync(all1.p, old1.p, used * sizeof(int), hipMemcpyDeviceToDevice, st));
                    SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
                }
                old0.free(); old1.free(); cap = ncap;
            }
            if (slab_total) {                                        // stream order keeps the slab's buffers intact until this has run
                SSFM_HIP_CHECK(ctx, hipMemcpyAsync(all0.p + used, d0, slab_total * sizeof(int), hipMemcpyDeviceToDevice, st));
                SSFM_HIP_CHECK(ctx, hipMemcpyAsync(all1.p + used, d1, slab_total * sizeof(int), hipMemcpyDeviceToDevice, st));
            }
            used += slab_total;
            return SSFM_OK;
        });
        if (rc) return rc;
        ctx->front_kernel_ms = ctx->match_kernel_ms;
        // 2. candidates: at least min_num_inliers matches and at least one (spherical_sfm_tools.cpp:353), in pair order
        std::vector<int32_t> cand, cf0, cf1, csrc, cptr(1, 0);
        for (int p = 0; p < num_pairs; p++) {
            const int c = mp[(size_t)p + 1] - mp[p];
            if (match_count) match_count[p] = c;
            if (c >= RO.min_num_inliers && c > 0) { cand.push_back(p); cf0.push_back(pair_frame0[p]); cf1.push_back(pair_frame1[p]); csrc.push_back(mp[p]); cptr.push_back(cptr.back() + c); }
        }
        const int K = (int)cand.size();
        if (K == 0) return SSFM_OK;
        // 3. LO-MSAC on the candidates, from the lists on the device; 4. inlier lists of the accepted pairs
        const size_t nf = (size_t)feat_ptr[num_frames];
        SSFM_HIP_CHECK(ctx, frays.alloc(std::max<size_t>(1, 3 * nf)));
        if (nf) SSFM_HIP_CHECK(ctx, hipMemcpyAsync(frays.p, feat_rays, 3 * nf * sizeof(double), hipMemcpyHostToDevice, st));
        SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));               // (the slabs' tables go up on another stream)
        H.ctx = ctx; H.who = who; H.five = five; H.t = t; H.E = E; H.d_idx0 = all0.p; H.d_idx1 = all1.p; H.list_len = (int)used; H.d_frays = frays.p;
        H.feat_ptr = feat_ptr; H.cf0 = cf0.data(); H.cf1 = cf1.data(); H.csrc = csrc.data(); H.cand = cand.data(); H.min_num_inliers = RO.min_num_inliers;
        H.pair_capacity = pair_capacity; H.inlier_capacity = inlier_capacity;
        H.accepted_pair = accepted_pair; H.R = R; H.num_inliers = num_inliers; H.inl_ptr = inl_ptr; H.inl_idx0 = inl_idx0; H.inl_idx1 = inl_idx1;
        std::vector<int32_t> nin((size_t)K, 0); std::vector<uint32_t> cst((size_t)2 * K, 0);
        rc = ransac_on_device_lists(ctx, num_frames, feat_ptr, K, cf0.data(), cf1.data(), cptr.data(), squared_inlier_threshold, RO, &H, nin.data(), cst.data(), five, who);
        if (rc) return rc;
        ctx->front_kernel_ms += ctx->ransac_kernel_ms;
        for (int k = 0; k < K; k++) {
            if (num_inliers_all) num_inliers_all[cand[k]] = nin[k];
            if (stats) { stats[2 * (size_t)cand[k]] = cst[2 * (size_t)k]; stats[2 * (size_t)cand[k] + 1] = cst[2 * (size_t)k + 1]; }
        }
        needed[0] = H.acc_run; needed[1] = H.inl_run;
        if (H.overflow) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": capacity too small; needed[0] / needed[1] hold the accepted pairs and the inlier matches");
        inl_ptr[H.acc_run] = (int32_t)H.inl_run;
        return SSFM_OK;
    };
    const int rc = body();
    (void)hipStreamSynchronize(st);
    H.release(); all0.free(); all1.free(); old0.free(); old1.free(); frays.free();
    return rc;
}

extern "C" int ssfm_pairwise_from_features(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, const double* feat_rays, int32_t num_pairs,
                                           const int32_t* pair_frame0, const int32_t* pair_frame1, const ssfm_match_options* match_opt,
                                           const ssfm_ransac_options* ransac_opt, double squared_inlier_threshold, int64_t pair_capacity, int64_t inlier_capacity,
                                           int64_t* needed, int32_t* accepted_pair, double* R, int32_t* num_inliers, int32_t* inl_ptr, int32_t* inl_idx0,
                                           int32_t* inl_idx1, int32_t* match_count, int32_t* num_inliers_all, uint32_t* stats) {
    return front_impl("ssfm_pairwise_from_features", false, ctx, num_frames, feat_ptr, descs, feat_rays, num_pairs, pair_frame0, pair_frame1, match_opt, ransac_opt,
                      squared_inlier_threshold, pair_capacity, inlier_capacity, needed, accepted_pair, R, nullptr, nullptr, num_inliers, inl_ptr, inl_idx0, inl_idx1, match_count,
                      num_inliers_all, stats);
}

// the same with ssfm_ransac5_batch_indexed as the estimator (the options go through ransac5_options inside ransac_on_device_lists; min_num_inliers, which also
// selects the candidates here, is not among the fields it overrides)
extern "C" int ssfm_pairwise5_from_features(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, const double* feat_rays, int32_t num_pairs,
                                            const int32_t* pair_frame0, const int32_t* pair_frame1, const ssfm_match_options* match_opt,
                                            const ssfm_ransac_options* ransac_opt, double squared_inlier_threshold, int64_t pair_capacity, int64_t inlier_capacity,
                                            int64_t* needed, int32_t* accepted_pair, double* R, double* t, double* E, int32_t* num_inliers, int32_t* inl_ptr,
                                            int32_t* inl_idx0, int32_t* inl_idx1, int32_t* match_count, int32_t* num_inliers_all, uint32_t* stats) {
    return front_impl("ssfm_pairwise5_from_features", true, ctx, num_frames, feat_ptr, descs, feat_rays, num_pairs, pair_frame0, pair_frame1, match_opt, ransac_opt,
                      squared_inlier_threshold, pair_capacity, inlier_capacity, needed, accepted_pair, R, t, E, num_inliers, inl_ptr, inl_idx0, inl_idx1, match_count,
                      num_inliers_all, stats);
}
