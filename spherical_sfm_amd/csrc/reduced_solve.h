// spherical_sfm_amd -- the reduced-system solve of the BA and pose-graph solvers (and of ssfm_band_solve_probe): banded Cholesky in Cuthill-McKee order + PCG
// refinement, or block-Jacobi PCG.  band_path.h decides which kernels a band gets and with what; here every kernel family has ONE launch function, and the
// substructured path (band_sub.h) is a sequence of named phases.  Lab variants (knobs.h) live inside the launch functions.
#pragma once
#include "ba_handle.h"
#include "band_path.h"

namespace ssfm {

// The one way a kernel with dynamic LDS is launched: a request above the 48 KB default raises the kernel's limit first (per solve, in front of the launch), then the
// launch inside a span of the profile.  Through a function pointer: default arguments of the kernel are spelled out by the caller.
template <typename... P>
static int raise_lds_limit(ssfm_ba_handle* h, void (*kernel)(P...), size_t lds) {
    if (lds > 48 * 1024) SSFM_HIP_CHECK(h->ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return SSFM_OK;
}
template <typename... P, typename... A>
static int launch_lds(ssfm_ba_handle* h, int kid, void (*kernel)(P...), dim3 grid, int threads, size_t lds, A... args) {
    if (int rc = raise_lds_limit(h, kernel, lds)) return rc;
    LAUNCH(h, kid, kernel, grid, threads, lds, args...);
    return SSFM_OK;
}

// segment / separator tables of the substructured factorisation (band_sub.h) and its work buffers
static int sub_upload(ssfm_ba_handle* h, int DC) {
    ssfm_ctx* ctx = h->ctx; hipStream_t st = ctx->stream; const BAFlat& F = h->F;
    if (F.band_block > 0) DC = F.band_block;                     // block size of the band (merged 3-dof pairs: 6)
    sub_build(F.comp_ptr, F.comp_twist, F.band, DC, h->sub, &F.rings);
    if (!F.wrap_ptr.empty()) { SSFM_HIP_CHECK(ctx, upload(h->wrap_ptr, F.wrap_ptr, st)); SSFM_HIP_CHECK(ctx, upload(h->wrap_blk, F.wrap_blk, st)); SSFM_HIP_CHECK(ctx, upload(h->wrap_row2, F.wrap_row2, st)); }
    if (!h->sub.enabled) return SSFM_OK;
    const BandSub& B = h->sub; const size_t Q = (size_t)F.band * DC, n = (size_t)(F.band_rows > 0 ? F.band_rows : F.Nc) * DC;
    SSFM_HIP_CHECK(ctx, upload(h->sub_tw_lo, B.tw_lo, st)); SSFM_HIP_CHECK(ctx, upload(h->sub_tw_hi, B.tw_hi, st)); SSFM_HIP_CHECK(ctx, upload(h->sub_tw_copy, B.tw_copy, st)); SSFM_HIP_CHECK(ctx, upload(h->sub_seg_given, B.seg_given, st));
    {   // back substitution mode of a segment: 0, or 1 / 2 for the two halves of a twisted component (band_kernels2.h: k_band_back_v2 solves the separator itself)
        std::vector<int> mode(B.seg_twist.size());
        for (size_t i = 0; i < mode.size(); i++) mode[i] = B.seg_twist[i] >= 0 ? 1 + (B.seg_twist[i] & 1) : 0;
        SSFM_HIP_CHECK(ctx, upload(h->sub_seg_mode, mode, st));
    }
    SSFM_HIP_CHECK(ctx, upload(h->sub_seg_lo, B.seg_lo, st)); SSFM_HIP_CHECK(ctx, upload(h->sub_seg_hi, B.seg_hi, st));
    SSFM_HIP_CHECK(ctx, upload(h->sub_seg_wend, B.seg_wend, st)); SSFM_HIP_CHECK(ctx, upload(h->sub_left, B.left_segs, st));
    SSFM_HIP_CHECK(ctx, upload(h->sub_sep_lo, B.sep_lo, st)); SSFM_HIP_CHECK(ctx, upload(h->sub_sep_rseg, B.sep_rseg, st));
    SSFM_HIP_CHECK(ctx, upload(h->sub_chain_ptr, B.chain_ptr, st));
    if (B.ntwist > 0) {
        SSFM_HIP_CHECK(ctx, upload(h->sub_fz_lo, B.fz_lo, st)); SSFM_HIP_CHECK(ctx, upload(h->sub_fz_hi, B.fz_hi, st)); SSFM_HIP_CHECK(ctx, upload(h->sub_fz_wend, B.fz_wend, st));
        SSFM_HIP_CHECK(ctx, upload(h->sub_fz_merge, B.fz_merge, st)); SSFM_HIP_CHECK(ctx, upload(h->sub_fz_await, B.fz_await, st)); SSFM_HIP_CHECK(ctx, upload(h->sub_fz_signal, B.fz_signal, st));
        SSFM_HIP_CHECK(ctx, h->sub_fz_flags.alloc((size_t)4 * B.ntwist)); SSFM_HIP_CHECK(ctx, hipMemsetAsync(h->sub_fz_flags.p, 0, (size_t)4 * B.ntwist * sizeof(int), st)); h->sub_fz_seq = 0;
    }
    if (B.nsep == 0) return SSFM_OK;                             // twisted components only: no spikes, no chain
    SSFM_HIP_CHECK(ctx, h->subZ.alloc(Q * n)); SSFM_HIP_CHECK(ctx, h->subD.alloc((size_t)B.nsep * Q * Q)); SSFM_HIP_CHECK(ctx, h->subT.alloc((size_t)B.nsep * 2 * Q));
    SSFM_HIP_CHECK(ctx, h->subF.alloc((size_t)(B.nsep + B.nchain) * Q * Q)); SSFM_HIP_CHECK(ctx, h->subL.alloc((size_t)B.nsep * Q * (Q + 1) / 2)); SSFM_HIP_CHECK(ctx, h->subW.alloc((size_t)B.nsep * 2 * Q));
    SSFM_HIP_CHECK(ctx, h->subC.alloc((size_t)B.nchain * Q * (Q + 1) / 2)); SSFM_HIP_CHECK(ctx, h->subTc.alloc((size_t)B.nchain * 2 * Q)); SSFM_HIP_CHECK(ctx, h->sub_flags.alloc((size_t)2 * B.nchain));
    SSFM_HIP_CHECK(ctx, hipMemsetAsync(h->sub_flags.p, 0, (size_t)2 * B.nchain * sizeof(int), st)); h->sub_seq = 0;
    if (B.nring > 0) {
        SSFM_HIP_CHECK(ctx, upload(h->ring_rec, B.ring_rec, st)); SSFM_HIP_CHECK(ctx, upload(h->ring_tail, B.ring_tail_ptr, st));
        SSFM_HIP_CHECK(ctx, h->crL.alloc((size_t)B.nsep * Q * Q)); SSFM_HIP_CHECK(ctx, h->crF.alloc((size_t)B.nsep * 2 * Q * Q)); SSFM_HIP_CHECK(ctx, h->crW.alloc((size_t)B.nsep * 2 * Q));
        SSFM_HIP_CHECK(ctx, h->crP.alloc((size_t)B.nsep * 2 * Q * Q)); SSFM_HIP_CHECK(ctx, h->crT.alloc((size_t)B.nsep * 4 * Q)); SSFM_HIP_CHECK(ctx, h->crE.alloc((size_t)B.nsep * Q * Q));
    }
    return SSFM_OK;
}

// ---- supernodal solver (snode.h): tables and buffers of a plan; the one launch that factors, substitutes and scatters
static int snode_upload(ssfm_ba_handle* h) {
    ssfm_ctx* ctx = h->ctx; hipStream_t st = ctx->stream;
    const SnodePlan& P = h->sn;
    if (!P.enabled) return SSFM_OK;
    SSFM_HIP_CHECK(ctx, upload(h->sn_half, P.half_rec, st)); SSFM_HIP_CHECK(ctx, upload(h->sn_step, P.step_rec.empty() ? std::vector<int>(SN_SREC, 0) : P.step_rec, st));
    SSFM_HIP_CHECK(ctx, upload(h->sn_node, P.node_cam, st)); SSFM_HIP_CHECK(ctx, upload(h->sn_tab, P.tab.empty() ? std::vector<int>(1, -1) : P.tab, st));
    SSFM_HIP_CHECK(ctx, h->sn_work.alloc(std::max<size_t>(P.work_doubles, 1))); SSFM_HIP_CHECK(ctx, h->sn_xchg.alloc(std::max<size_t>(P.xchg_doubles, 1)));
    SSFM_HIP_CHECK(ctx, h->sn_flags.alloc((size_t)std::max(P.nflags, 1)));
    SSFM_HIP_CHECK(ctx, hipMemsetAsync(h->sn_flags.p, 0, (size_t)std::max(P.nflags, 1) * sizeof(int), st));
    h->sn_seq = 0;
    return SSFM_OK;
}
template <int DC, int NR, bool RING>
static int snode_launch(ssfm_ba_handle* h, double* Y, size_t ystride, long long* stamps = nullptr) {
    const SnodePlan& P = h->sn;
    h->sn_seq++;
    return launch_lds(h, KID_SNODE, k_snode_solve<DC, NR, RING>, P.nhalf, SN_THREADS, P.lds_bytes(), h->S_val, h->rhs, h->Sfc, h->sn_half.p, h->sn_step.p, h->sn_node.p, h->sn_tab.p, h->cam_pos.p,
                      h->sn_work.p, h->sn_xchg.p, h->sn_flags.p, h->sn_seq, P.qtm, Y, ystride, reinterpret_cast<int*>(h->pcg.p + PCG_TOTAL), stamps);
}
// S y = [rhs | S_fc] by the supernodal solver; Y in the band-row layout of the right-hand sides (the second column only with a free focal length: it stays as
// k_finalize_gather left it otherwise, zero)
template <int DC>
static int snode_direct(ssfm_ba_handle* h, double* Y, size_t ystride, long long* stamps = nullptr) {
    const bool ring = h->sn.qtm > 0;
    if (h->F.focal_free) return ring ? snode_launch<DC, 2, true>(h, Y, ystride, stamps) : snode_launch<DC, 2, false>(h, Y, ystride, stamps);
    return ring ? snode_launch<DC, 1, true>(h, Y, ystride, stamps) : snode_launch<DC, 1, false>(h, Y, ystride, stamps);
}

// ---- the band solve ----------------------------------------------------------------------------------------------------------------------------
static int band_rows(const ssfm_ba_handle* h) { return h->F.band_rows > 0 ? h->F.band_rows : h->F.Nc; }      // rows of the band (>= cameras: twisted components)
static int* fail_word(const ssfm_ba_handle* h) { return reinterpret_cast<int*>(h->pcg.p + PCG_TOTAL); }       // the factorisation's failure flag, behind the PCG scalars

// the plan of this handle's band (band_path.h); DC = block size of the band (6 for merged 3-dof pairs)
static BandPath solve_path(const ssfm_ba_handle* h, int DC) {
    BandPathLab lab;      // the shipped library compiles the defaults in
    lab.chol_wave_map = SSFM_LAB_KNOB("SSFM_CHOL_WAVE_MAP", 1) != 0; lab.band_mfma = SSFM_LAB_KNOB("SSFM_BAND_MFMA", 0); lab.band_early = SSFM_LAB_KNOB("SSFM_BAND_EARLY", 0) != 0;
    lab.chol_fuse = SSFM_LAB_KNOB("SSFM_CHOL_FUSE", 0) != 0; lab.chain_pingpong = SSFM_LAB_KNOB("SSFM_CHAIN_PINGPONG", 1) != 0; lab.chain_twist = SSFM_LAB_KNOB("SSFM_CHAIN_TWIST", 1) != 0;
    lab.spike_nc = SSFM_LAB_KNOB("SSFM_SPIKE_NC", 0); lab.ring_roles = SSFM_LAB_KNOB("SSFM_RING_ROLES", 0);
    return band_path(DC, h->F.band, h->sub.enabled, band_packed_enabled(), h->ctx->num_cus, lab);
}

#ifdef SSFM_LAB
// Timing studies of the lab library.  SSFM_CHAIN_STAMPS=1: s_memtime stamps of the phases of one separator of the chain kernel, printed once (profiles/*_notes.md);
// the buffer stays, and with it the stamped kernel.  Declared in front of the launch, prints when it leaves scope behind it.
struct LabChainStamps {
    hipStream_t st; long long*& buf() { static long long* d = nullptr; return d; } int& state() { static int s = SSFM_LAB_KNOB("SSFM_CHAIN_STAMPS", 0) ? 1 : 0; return s; }
    explicit LabChainStamps(hipStream_t s) : st(s) {
        if (state() == 1) { (void)hipMalloc((void**)&buf(), 16 * sizeof(long long)); (void)hipMemsetAsync(buf(), 0, 16 * sizeof(long long), st); state() = 2; }
    }
    ~LabChainStamps() {
        if (state() != 2) return;
        long long hs[16]; (void)hipMemcpyAsync(hs, buf(), sizeof(hs), hipMemcpyDeviceToHost, st); (void)hipStreamSynchronize(st);
        std::fprintf(stderr, "[chain stamps, cycles] load E %lld | F solve %lld | t update + F store %lld | load D %lld | syrk %lld | chol J=0: diag %lld panel %lld trailing %lld | chol total %lld | stores %lld\n",
                     hs[1] - hs[0], hs[2] - hs[1], hs[3] - hs[2], hs[4] - hs[3], hs[5] - hs[4], hs[6] - hs[5], hs[7] - hs[6], hs[9] - hs[7], hs[8] - hs[5], hs[10] - hs[8]);
        state() = 3;
    }
};
// SSFM_RING_STAMPS=1: phase stamps of every ring elimination of the first solve, printed once: [loads | factorisation | stores + products]
struct LabRingStamps {
    hipStream_t st; int nsep, Q; long long* d = nullptr; int& state() { static int s = SSFM_LAB_KNOB("SSFM_RING_STAMPS", 0) ? 1 : 0; return s; }
    LabRingStamps(hipStream_t s, int nsep_, int Q_) : st(s), nsep(nsep_), Q(Q_) {
        if (state() == 1) { (void)hipMalloc((void**)&d, (size_t)4 * nsep * sizeof(long long)); (void)hipMemsetAsync(d, 0, (size_t)4 * nsep * sizeof(long long), st); state() = 2; }
    }
    ~LabRingStamps() {
        if (!d) return;
        std::vector<long long> hs((size_t)4 * nsep); (void)hipStreamSynchronize(st); (void)hipMemcpy(hs.data(), d, hs.size() * sizeof(long long), hipMemcpyDeviceToHost);
        double a = 0, bb = 0, c = 0; int cnt = 0;
        for (int q = 0; q < nsep; q++) if (hs[4 * q + 3] > 0) { a += hs[4 * q + 1] - hs[4 * q]; bb += hs[4 * q + 2] - hs[4 * q + 1]; c += hs[4 * q + 3] - hs[4 * q + 2]; cnt++; }
        if (cnt) std::fprintf(stderr, "[ring stamps, 100 MHz ticks] Q = %d, %d eliminations (parallel steps): loads %.0f | factorisation %.0f | stores + neighbour products %.0f\n", Q, cnt, a / cnt, bb / cnt, c / cnt);
        (void)hipFree(d); state() = 3;
    }
};
#endif

// Factorisation of `grid` row ranges [lo, hi) whose window runs on to wend (segments: the separator behind them), one workgroup each, the forward substitution of Y riding
// along: the square window or the packed one, as the path says.  merge: second copy of a twisted separator.  await2 / signal / flags / seq: the fused launch (lab).
template <int DC>
static int launch_chol(ssfm_ba_handle* h, const BandPath& p, int grid, const int* lo, const int* hi, const int* wend, const int* merge, double* Y,
                       const int* await2 = nullptr, const int* signal = nullptr, int* flags = nullptr, int seq = 0) {
    const int Nc = band_rows(h);
    if (p.packed()) {      // the packed-window kernel takes the same tables (no wave map: its roles sit in wave order)
        if constexpr (DC == 6) {
            auto k = p.factor == BAND_FACTOR_PACKED_T6 ? k_band_chol_v2p<2, 1, 2, 8, true> : p.npb == 1 ? k_band_chol_v2p<2, 3, 1, 8> : k_band_chol_v2p<2, 3, 2, 9>;
            return launch_lds(h, KID_BAND_CHOL, k, grid, p.chol_threads, p.chol_lds, h->band.p, h->Linv.p, Y, h->band_pairs.p, lo, hi, wend, merge, Nc, p.b, fail_word(h),
                              (const int*)nullptr, (const int*)nullptr, (int*)nullptr, 0);
        }
        return fail(h->ctx, SSFM_ERR_INVALID, "packed band window with blocks other than 6x6");
    }
    // the shipped library holds the VALU factorisation only: the matrix-core panel / trailing update and the early look-ahead were measured slower
    auto k = k_band_chol_v2<DC, 2, 0>;
#ifdef SSFM_LAB
    // matrix-core panel + trailing update (band_kernels2.h, MF): 6x6 blocks only.  Early look-ahead (MF bit 2 alone): the look-ahead wave computes X_1 and the update of the next
    // diagonal block before barrier A.  Measured in the lab (scripts/lab/chol_lab3.hip, same run): 89.8 against 79.9 us for 4 x 75 rows at half-width 10, 106.2 / 98.3 at 12,
    // 124.9 / 123.2 at 14 -- once the pivot test left the factorisation's chain the step is bound by the trailing waves, and the longer stretch in front of barrier A only delays them.
    constexpr int MFP = (DC == 6) ? 1 : 0, MFT = (DC == 6) ? 2 : 0, MFB = (DC == 6) ? 3 : 0;
    if (p.chol_early) k = k_band_chol_v2<DC, 2, 4>; else if (p.chol_mf == 3) k = k_band_chol_v2<DC, 2, MFB>; else if (p.chol_mf == 2) k = k_band_chol_v2<DC, 2, MFT>; else if (p.chol_mf == 1) k = k_band_chol_v2<DC, 2, MFP>;
#endif
    return launch_lds(h, KID_BAND_CHOL, k, grid, p.chol_threads, p.chol_lds, h->band.p, h->Linv.p, Y, h->band_pairs.p, lo, hi, wend, merge, Nc, p.b, fail_word(h), p.chol_map,
                      await2, signal, flags, seq);
}

// Back substitution behind an LDS-resident factorisation: one wave per (row range, right-hand side), one, two or three task sets per lane.  given: where a reversed
// segment reads its separator's solution; mode: twisted separators solved by the segment waves themselves (lab, SSFM_BACK_FUSE).
template <int DC>
static void launch_back_v2(ssfm_ba_handle* h, const BandPath& p, dim3 grid, double* Y, const int* lo, const int* hi, const int* wend, const int* given, const int* mode = nullptr) {
    auto k = p.back_sets == 3 ? k_band_back_v2<DC, 3> : p.back_sets == 2 ? k_band_back_v2<DC, 2> : k_band_back_v2<DC, 1>;
    LAUNCH(h, KID_BAND_BACK, k, grid, 64, 0, h->band.p, h->Linv.p, Y, lo, hi, wend, given, band_rows(h), p.b, mode);
}

// Spikes of the segments with a separator in front of them: one wave per (segment, nc columns)
template <int DC>
static void launch_spike(ssfm_ba_handle* h, const BandPath& p) {
    const BandSub& B = h->sub;
    const int nc = p.spike_cols(B.nleft);
    auto k = nc >= 4 ? k_sub_spike_fwd<DC, 4> : nc == 3 ? k_sub_spike_fwd<DC, 3> : nc == 2 ? k_sub_spike_fwd<DC, 2> : k_sub_spike_fwd<DC, 1>;
    LAUNCH(h, KID_SUB_SPIKE, k, dim3(B.nleft, (p.Q + nc - 1) / nc), 64, 0, h->band.p, h->Linv.p, h->subZ.p, h->sub_seg_lo.p, h->sub_seg_hi.p, h->sub_seg_wend.p, h->sub_left.p, band_rows(h), p.b);
}

// Separator blocks D and right-hand sides t on the matrix cores, operands straight from global memory, no atomics and no clears (band_sub.h 3b)
template <int DC>
static int launch_assemble(ssfm_ba_handle* h, const BandPath& p, double* Y, int max_rows) {
    const BandSub& B = h->sub; const int Nc = band_rows(h);
#ifdef SSFM_LAB
    if (SSFM_LAB_KNOB("SSFM_ASM_MFMA", 1) == 0) {      // the VALU kernel of round 1
        const int ntl = (p.Q + SUB_TS - 1) / SUB_TS, nz = std::max(1, std::min(64, (max_rows + 511) / 512));
        SSFM_HIP_CHECK(h->ctx, hipMemsetAsync(h->subD.p, 0, h->subD.n * sizeof(double), h->ctx->stream));
        SSFM_HIP_CHECK(h->ctx, hipMemsetAsync(h->subT.p, 0, h->subT.n * sizeof(double), h->ctx->stream));
        LAUNCH(h, KID_SUB_ASM, (k_sub_sep_assemble<DC, 2>), dim3(B.nsep, ntl * (ntl + 1) / 2, nz), 256, 0, h->band.p, h->subZ.p, Y, h->sub_sep_lo.p, h->sub_sep_rseg.p, h->sub_seg_lo.p, h->sub_seg_hi.p, Nc, p.b, h->subD.p, h->subT.p);
        return SSFM_OK;
    }
#endif
    (void)max_rows;
    const int tq = (p.Q + 15) / 16;
    LAUNCH(h, KID_SUB_ASM, (k_sub_sep_assemble_mfma<DC, 2>), B.nsep * (tq * (tq + 1) / 2 + tq), 64 * ASM_NW, 0, h->band.p, h->subZ.p, Y, h->sub_sep_lo.p, h->sub_sep_rseg.p, h->sub_seg_lo.p, h->sub_seg_hi.p, Nc, p.b, h->subD.p, h->subT.p);
    return SSFM_OK;
}

// Separator chains on the matrix cores (band_sub.h 4b), the 16x16 diagonal blocks factored and inverted there too; chains of three or more separators from both ends by
// two workgroups each while they all fit the device (BandPath::chain_two_sided)
template <int DC>
static int launch_chain(ssfm_ba_handle* h, const BandPath& p, double* Y) {
    const BandSub& B = h->sub; const int Nc = band_rows(h);
    const int tw = p.chain_two_sided(B.nchain) ? 1 : 0;
    auto k = k_sub_sep_chain_mfma<DC, 2>; int threads = 1024; long long* stamps = nullptr;
#ifdef SSFM_LAB
    // SSFM_CHAIN_MFMA=0: the VALU chain of round 1; SSFM_CHAIN_DIAG_MFMA=0: lane per row, no prefetch (round 2); SSFM_CHAIN_THREADS=512: eight waves with 256 registers each
    if (SSFM_LAB_KNOB("SSFM_CHAIN_MFMA", 1) == 0)
        return launch_lds(h, KID_SUB_CHAIN, k_sub_sep_chain<DC, 2>, B.nchain, 1024, p.chain_lds, h->subZ.p, h->subD.p, h->subT.p, h->sub_chain_ptr.p, h->sub_sep_lo.p, Nc, p.b, h->subF.p, h->subL.p, h->subW.p, Y, fail_word(h));
    LabChainStamps study(h->ctx->stream); stamps = study.buf();
    const bool diag_mfma = SSFM_LAB_KNOB("SSFM_CHAIN_DIAG_MFMA", 1) != 0;
    if (diag_mfma && SSFM_LAB_KNOB("SSFM_CHAIN_THREADS", 1024) == 512) { k = k_sub_sep_chain_mfma<DC, 2, true, true, 512>; threads = 512; }
    else if (diag_mfma && stamps) k = k_sub_sep_chain_mfma<DC, 2, true, true, 1024, true>;
    else if (!diag_mfma) k = k_sub_sep_chain_mfma<DC, 2, false, false>;
#endif
    h->sub_seq++;
    return launch_lds(h, KID_SUB_CHAIN, k, B.nchain * (tw ? 2 : 1), threads, p.chain_lds, h->subZ.p, h->subD.p, h->subT.p, h->sub_chain_ptr.p, h->sub_sep_lo.p, Nc, p.b, h->subF.p, h->subL.p, h->subW.p, Y,
                      fail_word(h), stamps, tw, B.nsep, h->subC.p, h->subTc.p, h->sub_flags.p, h->sub_seq, p.chain_pp);
}

// Rings (band_ring.h): the separator cycles by cyclic reduction -- one launch per parallel step down, ONE for the last few separators of every ring (their
// eliminations, the roots, their back substitutions), one per parallel step back up.  A step's launches share one kernel: its LDS limit is raised once, in front of them.
template <int DC>
static int launch_ring_eliminations(ssfm_ba_handle* h, const BandPath& p, size_t lds) {
    const BandSub& B = h->sub; long long* stamps = nullptr;
#ifdef SSFM_LAB
    LabRingStamps study(h->ctx->stream, B.nsep, p.Q); stamps = study.d;
#endif
    if (int rc = raise_lds_limit(h, k_ring_cr_elim<DC, 2>, lds)) return rc;
    for (int s = 0; s + 1 < (int)B.ring_step_ptr.size(); s++) {
        const int nodes = B.ring_step_ptr[s + 1] - B.ring_step_ptr[s];
        LAUNCH(h, KID_RING_ELIM, (k_ring_cr_elim<DC, 2>), dim3(nodes, p.ring_elim_roles(nodes)), p.ring_cr_threads, lds, h->ring_rec.p, B.ring_step_ptr[s], h->subZ.p, h->subD.p, h->subT.p,
               h->crL.p, h->crF.p, h->crW.p, h->crP.p, h->crT.p, h->crE.p, band_rows(h), p.b, fail_word(h), stamps);
    }
    return SSFM_OK;
}
template <int DC>
static int eliminate_rings(ssfm_ba_handle* h, const BandPath& p, double* Y) {
    const BandSub& B = h->sub; const int Nc = band_rows(h);
    const size_t le = ring_elim_lds_bytes(p.Q, 2), lb = ring_back_lds_bytes(p.Q, 2), lt = std::max(le, lb);
    if (int rc = launch_ring_eliminations<DC>(h, p, le)) return rc;
    if (int rc = launch_lds(h, KID_RING_TAIL, k_ring_cr_tail<DC, 2>, B.nring, p.ring_cr_threads, lt, h->ring_rec.p, h->ring_tail.p, h->subZ.p, h->subD.p, h->subT.p,
                            h->crL.p, h->crF.p, h->crW.p, h->crP.p, h->crT.p, h->crE.p, Y, Nc, p.b, fail_word(h))) return rc;
    if (int rc = raise_lds_limit(h, k_ring_cr_back<DC, 2>, lb)) return rc;
    for (int s = (int)B.ring_step_ptr.size() - 2; s >= 0; s--)
        LAUNCH(h, KID_RING_BACK, (k_ring_cr_back<DC, 2>), B.ring_step_ptr[s + 1] - B.ring_step_ptr[s], p.ring_back_threads, lb, h->ring_rec.p, B.ring_step_ptr[s], h->crL.p, h->crF.p, h->crW.p, Y, Nc, p.b);
    return SSFM_OK;
}

// Substructured: segments in parallel, spikes, separators (chains and rings), back substitution (band_sub.h)
template <int DC>
static int band_substructured(ssfm_ba_handle* h, const BandPath& p, double* Y) {
    const BandSub& B = h->sub;
    // EXPERIMENT, off (SSFM_BACK_FUSE=1): the separator of a twisted component back-substituted by the two segment waves themselves (k_band_back_v2's modes 1 / 2) instead
    // of by a launch of its own.  Measured at config 2 (scripts/lab/ab_backfuse.sh): one launch of 23.2-23.8 us against two of 12.1-12.6 (event brackets), 2.545-2.555 against
    // 2.530-2.546 ms per solve -- the second wave's redundant separator sweep and a second pipeline fill cost what the launch gap did
    const bool back_fuse = SSFM_LAB_KNOB("SSFM_BACK_FUSE", 0) != 0;
    // SSFM_CHOL_FUSE=1 (experiment, off): one launch for the segments AND the separators of twisted components, which then wait for their two halves
    // through flags in global memory.  Measured at config 2: 70.7 us for the fused launch against 2 x 35.2, 2.958 vs 2.919 ms per solve -- the fence + flag
    // hand-over costs what the launch boundary did (profiles/r02_notes.md)
    const bool fused = p.fused_factor(B.nseg, B.ntwist);
    int max_rows = 0; for (int sg : B.left_segs) max_rows = std::max(max_rows, (B.seg_hi[sg] - B.seg_lo[sg]) * DC);
    // 1. factor the segments (packed windows: no cut components at these widths, twisted halves only)
    if (fused) { h->sub_fz_seq++;
        if (int rc = launch_chol<DC>(h, p, B.nseg + B.ntwist, h->sub_fz_lo.p, h->sub_fz_hi.p, h->sub_fz_wend.p, h->sub_fz_merge.p, Y, h->sub_fz_await.p, h->sub_fz_signal.p, h->sub_fz_flags.p, h->sub_fz_seq)) return rc; }
    else if (int rc = launch_chol<DC>(h, p, B.nseg, h->sub_seg_lo.p, h->sub_seg_hi.p, h->sub_seg_wend.p, nullptr, Y)) return rc;
    if (B.nsep > 0) {
        launch_spike<DC>(h, p);                                                            // 2. spike forward
        if (int rc = launch_assemble<DC>(h, p, Y, max_rows)) return rc;                    // 3. assemble the separators
        if (B.nchain > 0) if (int rc = launch_chain<DC>(h, p, Y)) return rc;               // 4. eliminate the chains
        if (B.nring > 0) if (int rc = eliminate_rings<DC>(h, p, Y)) return rc;             // 5. eliminate the rings
    }
    if (B.ntwist > 0) {
        // 6. twisted components: both segments left their Schur updates in the separator and in its copy; the factorisation kernel merges them while loading its window and
        // solves the separator as a component of b rows; 7. its back substitution -- the reversed segment's reads that solution through seg_given
        if (!fused) if (int rc = launch_chol<DC>(h, p, B.ntwist, h->sub_tw_lo.p, h->sub_tw_hi.p, h->sub_tw_hi.p, h->sub_tw_copy.p, Y)) return rc;
        if (!back_fuse) launch_back_v2<DC>(h, p, dim3(B.ntwist, 2), Y, h->sub_tw_lo.p, h->sub_tw_hi.p, h->sub_tw_hi.p, nullptr);
    }
    if (B.nleft > 0)                                                                       // 8. apply left: the separators' solutions into the segments behind them
        if (int rc = launch_lds(h, KID_SUB_APPLY, k_sub_apply_left<DC, 2>, dim3(B.nleft, (max_rows + APPLY_ROWS - 1) / APPLY_ROWS), APPLY_ROWS * APPLY_SLICES, p.apply_lds(),
                                h->subZ.p, Y, h->sub_seg_lo.p, h->sub_seg_hi.p, h->sub_left.p, band_rows(h), p.b)) return rc;
    launch_back_v2<DC>(h, p, dim3(B.nseg, 2), Y, h->sub_seg_lo.p, h->sub_seg_hi.p, h->sub_seg_wend.p, h->sub_seg_given.p, back_fuse ? h->sub_seg_mode.p : nullptr);      // 9. back-substitute the segments
    return SSFM_OK;
}

// Factor the band in h->band (block-band Cholesky in Cuthill-McKee order) and solve for the two right-hand-side columns of Y
// (band order), in place.  Long components go through the substructured path when the plan holds one.
template <int DC>
static int band_direct(ssfm_ba_handle* h, double* Y) {
    const BandPath p = solve_path(h, DC);
    if (p.substructured) return band_substructured<DC>(h, p, Y);
    const int ncomp = (int)h->F.comp_ptr.size() - 1, Nc = band_rows(h);
    const int* lo = h->comp_ptr.p; const int* hi = lo + 1;
    if (p.lds_factor()) {      // LDS-resident: the window (square or packed) and the substitution rings fit the CU; one workgroup per component
        if (int rc = launch_chol<DC>(h, p, ncomp, lo, hi, hi, nullptr, Y)) return rc;
        launch_back_v2<DC>(h, p, dim3(ncomp, 2), Y, lo, hi, hi, nullptr);
        return SSFM_OK;
    }
    if (int rc = launch_lds(h, KID_BAND_CHOL, k_band_chol<DC, 2>, 1, 1024, p.chol_lds, h->band.p, h->Linv.p, Y, h->band_pairs.p, Nc, p.b, fail_word(h))) return rc;
    return launch_lds(h, KID_BAND_BACK, k_band_back<DC, 2>, 1, 256, p.subst_lds(2), h->band.p, h->Linv.p, Y, Nc, p.b);
}

// Second solve with the factor of band_direct (PCG refinement): forward + back substitution of the first column of Y with the stored
// factor.  needs_refactor is set when the path was the substructured one (no stand-alone substitution kernels: the caller rebuilds the band
// and calls band_direct again).
template <int DC>
static int band_resolve(ssfm_ba_handle* h, double* Y, bool* needs_refactor) {
    const BandPath p = solve_path(h, DC);
    const int ncomp = (int)h->F.comp_ptr.size() - 1, Nb = band_rows(h);
    *needs_refactor = p.needs_refactor();
    if (*needs_refactor) return SSFM_OK;
    if (p.factor == BAND_FACTOR_SQUARE) {
        if (int rc = launch_lds(h, KID_BAND_FWD, k_band_fwd_lds<DC, 1>, ncomp, 256, p.subst_lds(1), h->band.p, h->Linv.p, Y, h->comp_ptr.p, Nb, p.b)) return rc;
        launch_back_v2<DC>(h, p, dim3(ncomp, 1), Y, h->comp_ptr.p, h->comp_ptr.p + 1, h->comp_ptr.p + 1, nullptr);
        return SSFM_OK;
    }
    // (the packed window's factor too: its layout in global memory is the band's)
    if (int rc = launch_lds(h, KID_BAND_FWD, k_band_fwd<DC, 1>, 1, 256, p.subst_lds(1), h->band.p, h->Linv.p, Y, Nb, p.b)) return rc;
    return launch_lds(h, KID_BAND_BACK, k_band_back<DC, 1>, 1, 256, p.subst_lds(1), h->band.p, h->Linv.p, Y, Nb, p.b);
}

// Solve S y = rhs (block-CSR S with dense focal border) into h->px.
//   preconditioner 0: exact block-banded Cholesky in Cuthill-McKee order, then PCG refinement on the residual
//   preconditioner 1: block-Jacobi PCG (kept for comparison; needs ~10^3 iterations on a camera ring)
template <int DC>
static int solve_reduced(ssfm_ba_handle* h, double* host_pcg, int* iters_out, bool* ok_out, int stage) {
    // stage 0: enqueue the direct solve + residual check, no host sync (flags are read with the iteration scalars)
    // stage 1: flags are in host_pcg; run PCG refinement if the residual test failed
    // (block-Jacobi PCG, preconditioner 1, does everything in stage 0 with its own syncs)
    ssfm_ctx* ctx = h->ctx; hipStream_t st = ctx->stream;
    const BAFlat& F = h->F; const ssfm_ba_options& O = h->opt;
    const int Nc = F.Nc, n = Nc * DC, b = F.band;
    const int Nb = F.band_rows > 0 ? F.y_rows(DC) : Nc, nb = Nb * DC;      // rows (camera units) / stride of the right-hand-side columns in band order
    const double tol2 = O.pcg_tolerance * O.pcg_tolerance;
    if (O.preconditioner == 1) {
        if (stage == 1) return SSFM_OK;
        LAUNCH(h, KID_PCG_INIT, k_pcg_init<DC>, 1, 1024, 0, h->rhs, h->Minv.p, h->Sff.p, Nc, h->px.p, h->pr.p, h->pz.p, h->pp.p, h->pcg.p);
        int launched = 0; bool done = false;
        int chunk = std::max(8, h->pcg_prev_iters + 2);
        while (!done && launched < O.pcg_max_iterations) {
            const int todo = std::min(chunk, O.pcg_max_iterations - launched);
            for (int k = 0; k < todo; k++) {
                MATVEC(h, DC, h->pp.p);
                LAUNCH(h, KID_PCG_VECOPS, k_pcg_vecops<DC>, 1, 1024, 0, h->Minv.p, h->Sfc, h->Sff.p, Nc, tol2, h->px.p, h->pr.p, h->pz.p, h->pp.p, h->pq.p, h->pqpart.p, h->pcg.p);
            }
            launched += todo;
            SSFM_HIP_CHECK(ctx, hipMemcpyAsync(host_pcg, h->pcg.p, PCG_TOTAL * sizeof(double), hipMemcpyDeviceToHost, st));
            SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
            done = host_pcg[PCG_DONE] != 0.0;
            chunk = 8;
        }
        *iters_out = (int)host_pcg[PCG_ITERS];
        *ok_out = done && host_pcg[PCG_BREAKDOWN] == 0.0;
        return SSFM_OK;
    }
    // the band may use bigger blocks than S (two 3-dof cameras per 6x6 block row, ba_flatten.h: band_plan)
    const bool merged = F.band_block > 0 && F.band_block != DC;
    auto gather = [&]() {
        if (merged) LAUNCH(h, KID_BAND_GATHER, (k_band_gather<DC, true>), Nc, 256, 0, h->row_ptr.p, h->col_idx.p, h->S_val, h->cam_pos.p, h->cam_pos2.p, h->pair_dummy.p, Nc, b, h->band.p, h->wrap_ptr_p(), h->wrap_blk.p, h->wrap_row2.p);
        else LAUNCH(h, KID_BAND_GATHER, (k_band_gather<DC, false>), Nc, 256, 0, h->row_ptr.p, h->col_idx.p, h->S_val, h->cam_pos.p, h->cam_pos2.p, (const unsigned char*)nullptr, Nc, b, h->band.p, h->wrap_ptr_p(), h->wrap_blk.p, h->wrap_row2.p);
    };
    auto direct = [&](double* Y) -> int { return merged ? band_direct<6>(h, Y) : band_direct<DC>(h, Y); };
    if (stage == 0) {
    if (!h->zone_views) SSFM_HIP_CHECK(ctx, hipMemsetAsync(h->pcg.p, 0, (PCG_TOTAL + 1) * sizeof(double), st));      // flags + the factorisation fail word behind them
    if (!h->band_filled) {                                       // the BA path fills the band in its fused finalize kernel
        gather();
        hipLaunchKernelGGL(k_band_permute_rhs<DC>, dim3((n + 255) / 256), dim3(256), 0, st, h->rhs, h->Sfc, h->cam_pos.p, h->cam_pos2.p, h->pair_dummy.p, Nc, Nb, h->Yb.p);
    }
    h->band_filled = false;
    { const int rc = h->sn.enabled ? snode_direct<DC>(h, h->Yb.p, (size_t)nb) : direct(h->Yb.p); if (rc) return rc; }
    if (h->external_tail) { *iters_out = 0; *ok_out = true; return SSFM_OK; }
    // ---- focal arrow, then the residual check r = rhs - S x (PCG refinement with the factor as preconditioner while it is too large)
    if (F.sym_lower && h->tail.on) {
        const int phi_parts = !F.focal_free ? -1 : (Nc > 1024 ? std::min(64, (n + 2047) / 2048) : 0);      // -1: focal fixed, the arrow is empty (pqpart: Nc doubles, only used by the PCG mat-vec)
        if (phi_parts > 0) LAUNCH(h, KID_BAND_COMBINE, k_arrow_phi<DC>, phi_parts, 256, 0, h->Yb.p, h->Yb.p + nb, h->Sfc, h->cam_pos.p, Nc, h->pqpart.p);
        LAUNCH(h, KID_PCG_MATVEC, k_arrow_update<DC>, (Nc + 3) / 4, 512, 0, h->Yb.p, h->Yb.p + nb, h->Sfc, h->Sff.p, h->rhs + n, h->cam_pos.p, h->row_ptr.p, h->col_idx.p,
               h->trans_ptr.p, h->trans_blk.p, h->trans_row.p, h->S_val, Nc, h->px.p, h->pq.p, h->tail.cam, h->tail.focal, h->scale_cam.p, h->scale_f.p,
               h->tail.cam_c, h->tail.focal_c, h->tail.rot_c, h->scal.p, h->pqpart.p, phi_parts, h->col_pos.p, h->trans_pos.p, h->det ? h->det_lacc.p : (long long*)nullptr);
    } else if (F.sym_lower) {
        LAUNCH(h, KID_PCG_MATVEC, k_arrow_matvec<DC>, (Nc + 3) / 4, 256, 0, h->Yb.p, h->Yb.p + nb, h->Sfc, h->Sff.p, h->rhs + n, h->cam_pos.p, h->row_ptr.p, h->col_idx.p,
               h->trans_ptr.p, h->trans_blk.p, h->trans_row.p, h->S_val, Nc, h->px.p, h->pq.p);
    } else {
        LAUNCH(h, KID_BAND_COMBINE, k_band_combine<DC>, 1, 1024, 0, h->Yb.p, h->Yb.p + nb, h->Sfc, h->Sff.p, h->rhs + n, h->cam_pos.p, Nc, h->px.p);
        MATVEC(h, DC, h->px.p);
    }
    if (!h->tail.residual_later)     // (else: an extra workgroup of k_point_backsub does it)
        LAUNCH(h, KID_REF_VEC, k_ref_residual<DC>, 1, 1024, 0, h->rhs, h->pq.p, h->px.p, h->Sfc, h->Sff.p, Nc, tol2, h->pr.p, h->pcg.p);
    *iters_out = 0; *ok_out = true;
    return SSFM_OK;
    }
    int it = 0;
    { int fail_flag; std::memcpy(&fail_flag, &host_pcg[PCG_TOTAL], sizeof(int));
      if (fail_flag) { *iters_out = 0; *ok_out = false; return SSFM_OK; } }   // S not positive definite: invalid step
    while (host_pcg[PCG_DONE] == 0.0 && it < O.pcg_max_iterations) {
        hipLaunchKernelGGL(k_band_permute_rhs<DC>, dim3((n + 255) / 256), dim3(256), 0, st, h->pr.p, h->Sfc, h->cam_pos.p, h->cam_pos2.p, h->pair_dummy.p, Nc, Nb, h->Yr.p);
        bool refactor = h->sn.enabled;      // (the supernodal factor has no stand-alone substitution: the refinement path rebuilds the band and takes the band kernels)
        if (!refactor) { const int rc = merged ? band_resolve<6>(h, h->Yr.p, &refactor) : band_resolve<DC>(h, h->Yr.p, &refactor); if (rc) return rc; }
        if (refactor) {
            // the substructured factor has no stand-alone substitution kernels: rebuild the band from S and solve again (rare path)
            gather();
            const int rc = direct(h->Yr.p); if (rc) return rc;
        }
        LAUNCH(h, KID_BAND_COMBINE, k_band_combine<DC>, 1, 1024, 0, h->Yr.p, h->Yb.p + nb, h->Sfc, h->Sff.p, h->pr.p + n, h->cam_pos.p, Nc, h->pz.p);
        LAUNCH(h, KID_REF_VEC, k_ref_direction, 1, 1024, 0, h->pr.p, h->pz.p, n + 1, it == 0 ? 1 : 0, h->pp.p, h->pcg.p);
        MATVEC(h, DC, h->pp.p);
        LAUNCH(h, KID_REF_VEC, k_ref_step<DC>, 1, 1024, 0, h->Sfc, h->Sff.p, Nc, tol2, h->pp.p, h->pq.p, h->pqpart.p, h->px.p, h->pr.p, h->pcg.p);
        SSFM_HIP_CHECK(ctx, hipMemcpyAsync(host_pcg, h->pcg.p, PCG_TOTAL * sizeof(double), hipMemcpyDeviceToHost, st));
        SSFM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        it++;
    }
    *iters_out = it;
    *ok_out = host_pcg[PCG_DONE] != 0.0 && host_pcg[PCG_BREAKDOWN] == 0.0;
    return SSFM_OK;
}

}  // namespace ssfm
