// spherical_sfm_amd -- state shared by the device solvers: the BA handle (also used by the pose-graph solver as the
// container of its reduced system), its launch macros and the end-of-iteration hand-over to the host.  The reduced-system solve is reduced_solve.h.
#pragma once
#include "ba_flatten.h"
#include "ba_kernels.h"
#include "band_kernels2.h"
#include "band_kernels2p.h"
#include "band_sub.h"
#include "band_ring.h"
#include "snode.h"
#include "dev_buf.h"
#include "knobs.h"

namespace ssfm {

enum KernelId { KID_CAM_ROT, KID_POINT_LIN, KID_SCHUR_ROWS, KID_FINALIZE, KID_PCG_INIT, KID_PCG_MATVEC, KID_PCG_VECOPS,
                KID_CAM_UPDATE, KID_BACKSUB, KID_COST, KID_ALLREDUCE, KID_BAND_GATHER, KID_BAND_CHOL, KID_BAND_FWD, KID_BAND_BACK,
                KID_BAND_COMBINE, KID_REF_VEC, KID_CAM_SUMS, KID_SUB_SPIKE, KID_SUB_ASM, KID_SUB_CHAIN, KID_SUB_APPLY, KID_SCHUR_GRAM, KID_GRAM_BACKSUB, KID_RING_ELIM, KID_RING_BACK, KID_RING_TAIL, KID_DET_DECODE, KID_SNODE, KID_COUNT };
// names as rocprofv3 prints them (template arguments dropped)
static const char* kKernelNames[KID_COUNT] = {"k_cam_rot", "k_point_lin", "k_schur_pairs2", "k_finalize_gather", "k_pcg_init",
                                              "k_arrow_update", "k_pcg_vecops", "k_cam_update", "k_point_backsub",
                                              "k_point_cost", "rccl_allreduce", "k_band_gather", "k_band_chol_v2", "k_band_fwd_lds",
                                              "k_band_back_v2", "k_arrow_phi", "k_ref_vecops", "k_cam_sums2", "k_sub_spike_fwd",
                                              "k_sub_sep_assemble", "k_sub_sep_chain", "k_sub_apply_left", "k_schur_gram", "k_gram_backsub", "k_ring_cr_elim", "k_ring_cr_back", "k_ring_cr_tail", "k_det_decode", "k_snode_solve"};

}  // namespace ssfm

using namespace ssfm;

struct ssfm_ba_handle {
    ssfm_ctx* ctx = nullptr;
    int device = 0;              // cached at creation: destroy must not read through ctx (Python may finalise the context first)
    ssfm_ba_options opt;
    BAFlat F;
    int n_red = 0;                       // length of the all-reduced assembly buffer
    // device state
    DevBuf<double> cam_x, cam_c, cam_init, pts_x, pts_c, pts_init, focal3;   // focal3: [x, cand, init]
    DevBuf<double> rot_x, rot_c, scale_cam, scale_pt, scale_f, mask_cam, mask_pt, mask_f, diag_cam, diag_pt, diag_f;
    DevBuf<double> obs_xy; DevBuf<int> obs_cam, obs_pt, pt_start, cam_start, cam_obs, row_ptr, col_idx, diag_slot;
    // BA: scal, pcg and redbuf are views into one of two zones; an LM iteration works in one while the memset of the other (for the next
    // iteration) is already queued behind it, off the host's critical path
    DevBuf<double> zone; bool zone_views = false; size_t zone_len = 0, zone_nnz = 0, zone_n = 0;
    // SSFM_DETERMINISTIC=1 (det_acc.h): the assembly adds fixed-point limbs with integer atomics instead of doubles; k_det_decode turns them into the zone's doubles
    bool det = false; DevBuf<long long> det_limb, det_lacc; DevBuf<double> det_dfpart; size_t det_nacc = 0;
    // det_lacc: the long accumulators of the scalar block, LA_STRIDE words for every entry of every replica
    static constexpr size_t det_lacc_words = (size_t)SC_NSLOT * SC_TOTAL * LA_STRIDE;
    hipError_t clear_det_lacc() { return hipMemsetAsync(det_lacc.p, 0, det_lacc_words * sizeof(long long), ctx->stream); }
    void set_zone(int which) {
        scal.p = zone.p + (size_t)which * zone_len; pcg.p = scal.p + scal.n; redbuf.p = pcg.p + pcg.n;
        S_val = redbuf.p; rhs = S_val + zone_nnz; Udiag = rhs + (zone_n + 1); Sfc = Udiag + zone_n; gcraw = Sfc + zone_n; red_scal = gcraw + zone_n;
    }
    DevBuf<double> lmdev;                 // [go, radius] of the device-side step decision (k_publish -> speculative k_point_lin)
    DevBuf<double> Vs, Lf, gp, redbuf, Minv, Sff, px, pr, pz, pp, pq, pqpart, scal, pcg;
    DevBuf<double> band, Linv, Yb, Yr; DevBuf<int> cam_pos, band_pairs, band_fail, comp_ptr;
    // substructured factorisation of long components (band_sub.h); disabled => segments == components
    BandSub sub; DevBuf<int> sub_seg_lo, sub_seg_hi, sub_seg_wend, sub_left, sub_sep_lo, sub_sep_rseg, sub_chain_ptr, sub_tw_lo, sub_tw_hi, sub_tw_copy, sub_seg_given, sub_seg_mode;
    DevBuf<unsigned char> pair_dummy;    // merged 3-dof pairs: 1 = the partner slot of this camera is empty
    DevBuf<int> cam_pos2;                // second band row of the separator cameras of twisted components (-1 elsewhere); cam_pos holds BAND ROWS
    DevBuf<double> subZ, subD, subT, subF, subL, subW, subC, subTc; DevBuf<int> sub_flags, sub_fz_lo, sub_fz_hi, sub_fz_wend, sub_fz_merge, sub_fz_await, sub_fz_signal, sub_fz_flags; int sub_seq = 0, sub_fz_seq = 0;      // subC / subTc / flags: the two-sided chain's hand-over (band_sub.h 4b)
    DevBuf<int> col_pos, trans_pos;      // band row of the column camera of every stored / transposed block (k_arrow_update)
    // rings (round 5, band_ring.h): wrap table of the gather kernels, cyclic-reduction schedule, per-separator factor / coupling / right-hand-side blocks
    DevBuf<int> wrap_ptr, wrap_blk, wrap_row2, ring_rec, ring_tail; DevBuf<double> crL, crF, crW, crP, crT, crE;
    const int* wrap_ptr_p() const { return wrap_ptr.n ? wrap_ptr.p : nullptr; }
    // supernodal ring / chain solver of the reduced system (snode.h): plan, tables, factor workspace, the halves' exchange buffers and flags
    SnodePlan sn; DevBuf<int> sn_half, sn_step, sn_node, sn_tab, sn_flags; DevBuf<double> sn_work, sn_xchg; int sn_seq = 0;
    DevBuf<int> trans_ptr, trans_blk, trans_row, pair_j, pair_j2, pair_p, batch_slot, cam_batch_ptr, chunk_cam, chunk_b0, chunk_b1, cam_obs_pt, cs_task_cam, cs_task_q0, cs_task_q1;
    double *S_val = nullptr, *rhs = nullptr, *Udiag = nullptr, *Sfc = nullptr, *gcraw = nullptr, *red_scal = nullptr;
    double focal_host = 0, t_flatten_s = 0;
    double* host_sp = nullptr;           // pinned read-back buffer of the LM loop
    double* host_pub = nullptr;          // = ctx->host_pub once publish_alloc ran (k_publish target, coherent pinned memory)
    bool scale_ready = false;
    bool band_filled = false;            // set by k_finalize_gather for the next solve_reduced call
    // set by the LM loop for the next solve_reduced call: the candidate cameras are produced by the arrow kernel (k_arrow_update)
    struct { bool on = false, residual_later = false; const double *cam = nullptr, *focal = nullptr; double *cam_c = nullptr, *focal_c = nullptr, *rot_c = nullptr; } tail;
    DevBuf<int> gr_rec; DevBuf<unsigned char> pt_grouped;     // signature groups of k_schur_gram (ba_flatten.h)
    // atomics-free Gram emission (round 6): the tasks' partial blocks / vectors and the fold lists of k_finalize_gather; gram_fold = the path is in use
    DevBuf<double> gram_part; DevBuf<int> gpart_off, fold_slot_ptr, fold_slot_src; bool gram_fold = false;
    DevBuf<int> pub_ticket;              // arrival counter of the fused hand-over in k_point_backsub (zero between launches)
    int pcg_prev_iters = 16;
    bool external_tail = false;          // the caller runs its own focal arrow / residual check after the direct solve (rotavg_solver.hip: k_rot_step, k_rot_eval)
    // profiling
    bool profile = false;
    std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
    struct Span { int kid; hipEvent_t a, b; };
    std::vector<Span> spans;
    int64_t k_launches[KID_COUNT]; double k_ms[KID_COUNT];
    hipEvent_t phase_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t x0_ev = nullptr;          // behind the copy of |x_0|^2 at a solve's start: the host reads it when the first tail is enqueued, not before the first kernels

    hipEvent_t get_event() {
        if (ev_used == ev_pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); ev_pool.push_back(e); }
        return ev_pool[ev_used++];
    }
    void span_begin(int kid) { if (!profile) return; Span s{kid, get_event(), get_event()}; (void)hipEventRecord(s.a, ctx->stream); spans.push_back(s); }
    void span_end() { if (!profile) return; (void)hipEventRecord(spans.back().b, ctx->stream); }
    void resolve_spans() {
        for (auto& s : spans) { float ms = 0; if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { k_ms[s.kid] += ms; k_launches[s.kid]++; } }
        spans.clear(); ev_used = 0;
    }
    void free_all() {
        cam_x.free(); cam_c.free(); cam_init.free(); pts_x.free(); pts_c.free(); pts_init.free(); focal3.free();
        rot_x.free(); rot_c.free(); scale_cam.free(); scale_pt.free(); scale_f.free(); mask_cam.free(); mask_pt.free(); mask_f.free();
        diag_cam.free(); diag_pt.free(); diag_f.free(); obs_xy.free(); obs_cam.free(); obs_pt.free(); pt_start.free();
        cam_start.free(); cam_obs.free(); row_ptr.free(); col_idx.free(); diag_slot.free(); Vs.free(); Lf.free(); gp.free();
        lmdev.free(); band.free(); Linv.free(); Yb.free(); Yr.free(); cam_pos.free(); band_pairs.free(); band_fail.free(); comp_ptr.free();
        sub_seg_lo.free(); sub_seg_hi.free(); sub_seg_wend.free(); sub_left.free(); sub_sep_lo.free(); sub_sep_rseg.free(); sub_chain_ptr.free(); sub_tw_lo.free(); sub_tw_hi.free(); sub_tw_copy.free(); sub_seg_given.free(); sub_seg_mode.free(); cam_pos2.free(); pair_dummy.free();
        subZ.free(); subD.free(); subT.free(); subF.free(); subL.free(); subW.free(); subC.free(); subTc.free(); sub_flags.free(); sub_fz_lo.free(); sub_fz_hi.free(); sub_fz_wend.free(); sub_fz_merge.free(); sub_fz_await.free(); sub_fz_signal.free(); sub_fz_flags.free();
        col_pos.free(); trans_pos.free(); trans_ptr.free(); trans_blk.free(); trans_row.free(); pair_j.free(); pair_j2.free(); pair_p.free(); batch_slot.free(); cam_batch_ptr.free(); chunk_cam.free(); chunk_b0.free(); chunk_b1.free(); cam_obs_pt.free(); cs_task_cam.free(); cs_task_q0.free(); cs_task_q1.free();
        if (zone_views) { scal.p = nullptr; pcg.p = nullptr; redbuf.p = nullptr; zone_views = false; }
        pub_ticket.free(); gr_rec.free(); pt_grouped.free();
        gram_part.free(); gpart_off.free(); fold_slot_ptr.free(); fold_slot_src.free(); gram_fold = false;
        sn_half.free(); sn_step.free(); sn_node.free(); sn_tab.free(); sn_flags.free(); sn_work.free(); sn_xchg.free(); sn.enabled = false;
        wrap_ptr.free(); wrap_blk.free(); wrap_row2.free(); ring_rec.free(); ring_tail.free(); crL.free(); crF.free(); crW.free(); crP.free(); crT.free(); crE.free();
        zone.free(); redbuf.free(); Minv.free(); Sff.free(); px.free(); pr.free(); pz.free(); pp.free(); pq.free(); pqpart.free(); scal.free(); pcg.free();
        if (host_sp) { (void)hipHostFree(host_sp); host_sp = nullptr; }
        host_pub = nullptr;
        for (auto e : ev_pool) (void)hipEventDestroy(e);
        ev_pool.clear();
        for (auto& e : phase_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (x0_ev) { (void)hipEventDestroy(x0_ev); x0_ev = nullptr; }
    }
};

namespace ssfm {

#define MATVEC(h, DCV, vec)                                                                                                   \
    do {                                                                                                                   \
        if ((h)->F.sym_lower)                                                                                              \
            LAUNCH(h, KID_PCG_MATVEC, k_sym_matvec<DCV>, ((h)->F.Nc + 3) / 4, 256, 0, (h)->row_ptr.p, (h)->col_idx.p, (h)->trans_ptr.p, \
                   (h)->trans_blk.p, (h)->trans_row.p, (h)->S_val, (h)->Sfc, vec, (h)->F.Nc, (h)->pcg.p, (h)->pq.p, (h)->pqpart.p);       \
        else                                                                                                               \
            LAUNCH(h, KID_PCG_MATVEC, k_pcg_matvec<DCV>, ((h)->F.Nc + 3) / 4, 256, 0, (h)->row_ptr.p, (h)->col_idx.p, (h)->S_val,       \
                   (h)->Sfc, vec, (h)->F.Nc, (h)->pcg.p, (h)->pq.p, (h)->pqpart.p);                                         \
    } while (0)
#define LAUNCH(h, kid, kernel, grid, block, shmem, ...)                                   \
    do {                                                                                  \
        (h)->span_begin(kid);                                                             \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), shmem, (h)->ctx->stream, __VA_ARGS__); \
        (h)->span_end();                                                                  \
    } while (0)

static int allreduce(ssfm_ba_handle* h, double* buf, size_t n, ncclRedOp_t op) {
    if (!h->ctx->collective) return SSFM_OK;
    // TIMING EXPERIMENT ONLY (bench.py --gpus N, `timing_without_collective`; switched on by ssfm_debug_timing_skip_collectives, which warns on stderr -- no
    // environment variable can do this): every rank solves its own shard without the reductions -- the results are meaningless, the kernels and their sizes are
    // those of the sharded solve, so the difference to the real run prices the collectives
    if (h->ctx->timing_skip_collectives) return SSFM_OK;
    h->span_begin(KID_ALLREDUCE);
    const int rc = ctx_allreduce(h->ctx, buf, n, op);
    h->span_end();
    return rc;
}

// ---- end-of-iteration hand-over to the host without a copy or a stream synchronisation (k_publish, ba_kernels.h) ----
static bool lm_poll() {                                             // read per solve (tests switch it within one process)
    const char* e = std::getenv("SSFM_LM_POLL");
    return !(e && std::atoi(e) == 0);
}
// false: no coherent pinned block to be had -- the caller falls back to the copy + stream synchronisation hand-over
static bool publish_alloc(ssfm_ba_handle* h) {
    ssfm_ctx* ctx = h->ctx;
    if (!ctx->host_pub) {
        if (hipHostMalloc((void**)&ctx->host_pub, 32 * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError(); ctx->host_pub = nullptr; return false;
        }
        std::memset(ctx->host_pub, 0, 32 * sizeof(double));
    }
    h->host_pub = ctx->host_pub;
    return true;
}
static void publish(ssfm_ba_handle* h, const LmGate* gate = nullptr, double* spec = nullptr, unsigned det_kmask = 0) {
    LmGate g; std::memset(&g, 0, sizeof(g)); if (gate) g = *gate;
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(SC_TOTAL * 64), 0, h->ctx->stream, h->scal.p, h->pcg.p, h->host_pub, ++h->ctx->pub_seq, g, spec,
                       (h->det && det_kmask) ? h->det_lacc.p : (long long*)nullptr, det_kmask);
}
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::atomic_signal_fence(std::memory_order_seq_cst);
#endif
}
// spin until the sequence number of the last publish() shows up; now and then ask the stream whether it is still alive
static int wait_published(ssfm_ba_handle* h) {
    ssfm_ctx* ctx = h->ctx;
    volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(h->host_pub + SC_TOTAL + PCG_TOTAL + 1);
    const unsigned long long want = ctx->pub_seq;
    unsigned spins = 0;
    while (*flag != want) {
        cpu_relax();
        if ((++spins & 0xFFFFu) == 0) {                          // every millisecond or so
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q == hipSuccess) { if (*flag == want) break; return fail(ctx, SSFM_ERR_HIP, "an LM iteration ended without publishing its scalars"); }
            if (q != hipErrorNotReady) return fail(ctx, SSFM_ERR_HIP, hipGetErrorString(q));
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return SSFM_OK;
}

}  // namespace ssfm
