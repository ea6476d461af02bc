// spherical_sfm_amd -- general view graphs: the triplet filter of the reference's non-sequential branch and a rotation initialisation over any graph.
//
//   ssfm_triplet_filter       filter_image_matches, examples/spherical_sfm_tools.cpp:1031-1082: an O(E^3) host loop there, a sparse join here.  The host sorts the
//                             edges into a CSR by index0 (view_graph_host.h).  One wave owns one first edge i = (a, b); its lanes stride over out(b); a lane forms
//                             M = Ri Rj once, finds the edges (a, c) of out(a) by binary search (a range: duplicates) and evaluates |so3ln(M Rk^T)| per hit.  Flags are
//                             plain stores of 1, the per-edge triplet count is one store of one lane, nothing is accumulated across lanes in floating point: the
//                             result depends on the inputs alone.  Records come from a second launch that knows its offsets (exclusive scan of the counts on the host,
//                             a wave prefix sum of the hit counts per chunk of 64 j): no atomics.
//   ssfm_view_graph_tree      breadth-first spanning tree, host code (view_graph_host.h)
//   ssfm_focal_search_graph   ssfm_focal_search (ransac.hip) with the rotations chained along that tree instead of along the matches (k-1, k): k_focal_trials_graph
//                             walks the tree level by level, the lanes share a level's nodes, one barrier between levels.
// GraphOptim (initialize_rotations_gopt) is third party and stays out; the tree + the robust rotation averaging that follows is what this project defines instead.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "ransac_device.h"
#include "view_graph_host.h"

namespace ssfm {

// What one wave does for the first edge at list position i.  REC = false: flags + count.  REC = true: the records, at rec_base + (position within the edge's triplets).
template <bool REC>
__device__ __forceinline__ void triplet_wave(int i, int lane, const int* __restrict__ row_ptr, const int* __restrict__ s0, const int* __restrict__ s1,
                                             const int* __restrict__ perm, const int* __restrict__ inv, const double* __restrict__ Rs, double thresh, int order,
                                             int* __restrict__ good, long long* __restrict__ tri_count, long long rec_base, long long rec_cap,
                                             int* __restrict__ rec_edges, double* __restrict__ rec_err) {
    const int p = inv[i], a = s0[p], b = s1[p];                         // wave-uniform; the host has checked every index against [0, num_cameras)
    const int jb = row_ptr[b], je = row_ptr[b + 1], kb = row_ptr[a], ke = row_ptr[a + 1];
    double Ri[9];
#pragma unroll
    for (int q = 0; q < 9; q++) Ri[q] = Rs[9 * (size_t)p + q];
    long long cnt = 0, base = rec_base;
    bool hit_i = false;
    for (int j0 = jb; j0 < je; j0 += 64) {
        const int pj = j0 + lane;
        int lo = 0, hi = 0;
        double M[9];
        if (pj < je) {
            const int c = s1[pj];
            lo = view_graph_bound<false>(s1, kb, ke, c);
            hi = view_graph_bound<true>(s1, lo, ke, c);
            if (hi > lo) triplet_pair_product(Ri, Rs + 9 * (size_t)pj, order, M);
        }
        const int h = hi - lo;
        if (REC) {
            int incl = h;                                                // wave prefix sum of the hit counts of this chunk
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
            const long long first = base + (incl - h);
            for (int t = 0; t < h; t++) {
                const long long at = first + t;
                if (at < rec_cap) {
                    rec_edges[3 * at] = i; rec_edges[3 * at + 1] = perm[pj]; rec_edges[3 * at + 2] = perm[lo + t];
                    rec_err[at] = triplet_error(M, Rs + 9 * (size_t)(lo + t));
                }
            }
            base += __shfl(incl, 63, 64);
        } else {
            bool hit_j = false;
            for (int pk = lo; pk < hi; pk++)
                if (triplet_error(M, Rs + 9 * (size_t)pk) < thresh) { good[perm[pk]] = 1; hit_j = true; }
            if (hit_j) { good[perm[pj]] = 1; hit_i = true; }
            cnt += h;
        }
    }
    if (!REC) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        const bool any = __any(hit_i);
        if (lane == 0) { tri_count[i] = cnt; if (any) good[i] = 1; }
    }
}

__global__ void __launch_bounds__(256)
k_triplet_filter(int E, const int* __restrict__ row_ptr, const int* __restrict__ s0, const int* __restrict__ s1, const int* __restrict__ perm,
                 const int* __restrict__ inv, const double* __restrict__ Rs, double thresh, int order, int* __restrict__ good, long long* __restrict__ tri_count) {
    const long long w = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= E) return;
    triplet_wave<false>((int)w, threadIdx.x & 63, row_ptr, s0, s1, perm, inv, Rs, thresh, order, good, tri_count, 0, 0, nullptr, nullptr);
}

// first edges i_lo .. i_hi; rec_off[i]: the number of triplets of all first edges before i (exclusive scan of tri_count); the buffers hold the records
// slab_base .. slab_base + rec_cap
__global__ void __launch_bounds__(256)
k_triplet_records(int i_lo, int i_hi, const int* __restrict__ row_ptr, const int* __restrict__ s0, const int* __restrict__ s1, const int* __restrict__ perm,
                  const int* __restrict__ inv, const double* __restrict__ Rs, int order, const long long* __restrict__ rec_off, long long slab_base, long long rec_cap,
                  int* __restrict__ rec_edges, double* __restrict__ rec_err) {
    const long long w = (long long)i_lo + (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= i_hi) return;
    triplet_wave<true>((int)w, threadIdx.x & 63, row_ptr, s0, s1, perm, inv, Rs, 0.0, order, nullptr, nullptr, rec_off[w] - slab_base, rec_cap, rec_edges, rec_err);
}

// k_focal_trials (ransac.hip) with the tree walk in place of the chain: one workgroup per trial focal, the same transform_image_matches step, the same get_cost.
// tree_*: the spanning tree in visiting order (position 0 = the root), level_ptr delimits its levels.
__global__ void __launch_bounds__(256)
k_focal_trials_graph(int n, int E, const int* __restrict__ e0, const int* __restrict__ e1, int num_levels, const int* __restrict__ level_ptr,
                     const int* __restrict__ tree_node, const int* __restrict__ tree_parent, const int* __restrict__ tree_edge, const int* __restrict__ tree_rev,
                     const double* __restrict__ Es /*[E*9] row-major*/, int inward, double focal_guess, const double* __restrict__ focals,
                     double* __restrict__ rnew_all /*[trials*E*3]*/, double* __restrict__ x_all /*[trials*n*3]*/,
                     double* __restrict__ rot_all /*[trials*n*9] row-major*/, double* __restrict__ costs) {
    __shared__ double red[4]; __shared__ double s_scale;
    const int trial = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const double f = focals[trial], tf = f / focal_guess;
    double* rnew = rnew_all + (size_t)trial * E * 3; double* x = x_all + (size_t)trial * n * 3; double* rot = rot_all + (size_t)trial * n * 9;
    double mx = 0.0;
    for (int e = tid; e < E; e += nt) {
        double En[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) En[3 * i + j] = Es[9 * (size_t)e + 3 * i + j] * ((i < 2) ? tf : 1.0) * ((j < 2) ? tf : 1.0);
        double r[3]; decompose_E_dev(En, inward != 0, r);
        // the reference stores so3exp(r_new) and get_cost takes so3ln of it again
        double Rm[9], rr[3]; so3exp(r, Rm); so3ln(Rm, rr);
        rnew[3 * e] = rr[0]; rnew[3 * e + 1] = rr[1]; rnew[3 * e + 2] = rr[2];
        mx = fmax(mx, norm3(rr));
    }
    for (int i = tid; i < n; i += nt) { double* dst = rot + 9 * (size_t)i; for (int k = 0; k < 9; k++) dst[k] = (k % 4 == 0) ? 1.0 : 0.0; }     // the root and every unreached camera
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) { double m = 0; for (int w = 0; w < (nt >> 6); w++) m = fmax(m, red[w]); s_scale = 1.0 / m; }
    // level by level: a node's parent was written one level earlier (global writes of this block are visible to it after the barrier)
    for (int l = 1; l < num_levels; l++) {
        for (int k = level_ptr[l] + tid; k < level_ptr[l + 1]; k += nt) {
            const int e = tree_edge[k];
            double Rm[9], Rp[9], Rn[9];
            so3exp(rnew + 3 * e, Rm);
            for (int q = 0; q < 9; q++) Rp[q] = rot[9 * (size_t)tree_parent[k] + q];
            if (tree_rev[k]) mat3_mul_at(Rm, Rp, Rn); else mat3_mul(Rm, Rp, Rn);
            double* dst = rot + 9 * (size_t)tree_node[k];
            for (int q = 0; q < 9; q++) dst[q] = Rn[q];
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) so3ln(rot + 9 * (size_t)i, x + 3 * i);
    __syncthreads();
    const double scale = s_scale;
    double c = 0.0;
    for (int e = tid; e < E; e += nt) {
        double Rm[9], R0[9], R1[9], A[9], C[9], res[3];
        angle_axis_to_matrix(rnew + 3 * e, Rm); angle_axis_to_matrix(x + 3 * e0[e], R0); angle_axis_to_matrix(x + 3 * e1[e], R1);
        mat3_mul_bt(R1, R0, A); mat3_mul_bt(A, Rm, C);
        matrix_to_angle_axis(C, res);
        const double s2 = scale * scale * (res[0] * res[0] + res[1] * res[1] + res[2] * res[2]);
        double rho0, rho1; robust_loss(2, 0.03, s2, rho0, rho1);
        c += 0.5 * rho0;
    }
    c = wave_sum(c);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) { double t = 0; for (int w = 0; w < (nt >> 6); w++) t += red[w]; costs[trial] = t; }
}

}  // namespace ssfm
using namespace ssfm;

// the device buffers of one record slab stay within the bound the match path uses for its slot buffer (match.hip: 64 MB); SSFM_TRIPLET_SLAB_RECORDS (read at
// every call, like SSFM_MATCH_SLAB_PAIRS) overrides the record count of a slab, so that a small problem can walk the multi-slab path
static const size_t kRecordSlabBytes = (size_t)64 << 20;

// a failed HIP call inside an entry point: wait for what is in flight, give the temporaries back (`release` of the enclosing function), report
#define VG_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipStreamSynchronize(st); release(); return fail(ctx, SSFM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)

extern "C" int ssfm_triplet_filter(ssfm_ctx* ctx, int32_t num_cameras, int32_t num_edges, const int32_t* index0, const int32_t* index1, const double* rel_rotations,
                                   double err_thresh_rad, int32_t order, uint8_t* good_out, int64_t* num_triplets_out, int64_t max_records,
                                   int32_t* triplet_edges_out, double* triplet_err_out) {
    const char* who = "ssfm_triplet_filter";
    if (num_cameras < 0 || num_edges < 0 || (num_edges > 0 && (!index0 || !index1 || !rel_rotations || !good_out)) || max_records < 0 ||
        (order != SSFM_TRIPLET_ORDER_REFERENCE && order != SSFM_TRIPLET_ORDER_COMPOSED) || !(err_thresh_rad == err_thresh_rad) ||
        ((triplet_edges_out != nullptr) != (triplet_err_out != nullptr)))
        return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": bad arguments");
    ViewGraphCsr G;
    if (!view_graph_csr(num_cameras, num_edges, index0, index1, G))
        return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": camera index out of range");             // before anything is launched
    if (!ctx) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": ctx is null");
    if (ctx->collective) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": the context carries a communicator; this call is single-GPU");
    if (num_triplets_out) *num_triplets_out = 0;
    if (num_edges == 0) return SSFM_OK;
    const int E = num_edges;
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<double> Rs((size_t)9 * E);                                                                  // sorted order, row-major
    for (int p = 0; p < E; p++) cm_to_rm(rel_rotations + 9 * (size_t)G.perm[(size_t)p], &Rs[9 * (size_t)p]);
    DevBuf<int> d_row, d_s0, d_s1, d_perm, d_inv, d_good, d_rec; DevBuf<double> d_R, d_err; DevBuf<long long> d_cnt, d_off;
    auto release = [&]() { d_row.free(); d_s0.free(); d_s1.free(); d_perm.free(); d_inv.free(); d_good.free(); d_rec.free(); d_R.free(); d_err.free(); d_cnt.free(); d_off.free(); };
    VG_CHECK(upload(d_row, G.row_ptr, st)); VG_CHECK(upload(d_s0, G.s0, st)); VG_CHECK(upload(d_s1, G.s1, st)); VG_CHECK(upload(d_perm, G.perm, st));
    VG_CHECK(upload(d_inv, G.inv, st)); VG_CHECK(upload(d_R, Rs, st));
    VG_CHECK(d_good.alloc(E)); VG_CHECK(d_cnt.alloc(E));
    VG_CHECK(hipMemsetAsync(d_good.p, 0, (size_t)E * sizeof(int), st));
    const unsigned blocks = (unsigned)(((size_t)E + 3) / 4);
    hipLaunchKernelGGL(k_triplet_filter, dim3(blocks), dim3(256), 0, st, E, d_row.p, d_s0.p, d_s1.p, d_perm.p, d_inv.p, d_R.p, err_thresh_rad, order, d_good.p, d_cnt.p);
    VG_CHECK(hipGetLastError());
    std::vector<int> hgood((size_t)E); std::vector<long long> hcnt((size_t)E);
    VG_CHECK(hipMemcpyAsync(hgood.data(), d_good.p, (size_t)E * sizeof(int), hipMemcpyDeviceToHost, st));
    VG_CHECK(hipMemcpyAsync(hcnt.data(), d_cnt.p, (size_t)E * sizeof(long long), hipMemcpyDeviceToHost, st));
    VG_CHECK(hipStreamSynchronize(st));
    for (int e = 0; e < E; e++) good_out[e] = hgood[(size_t)e] ? 1 : 0;
    std::vector<long long> off((size_t)E + 1, 0);
    for (int e = 0; e < E; e++) off[(size_t)e + 1] = off[(size_t)e] + hcnt[(size_t)e];                       // int64 on the host
    if (num_triplets_out) *num_triplets_out = (int64_t)off[(size_t)E];
    const long long want = std::min<long long>(off[(size_t)E], max_records);
    if (triplet_edges_out && want > 0) {
        VG_CHECK(upload(d_off, off, st));
        long long slab_records = (long long)(kRecordSlabBytes / (3 * sizeof(int) + sizeof(double)));
        if (const char* e = getenv("SSFM_TRIPLET_SLAB_RECORDS")) slab_records = std::max<long long>(1, atoll(e));
        int i_lo = 0;
        while (i_lo < E && off[(size_t)i_lo] < want) {
            // the first edges whose records fit the slab (at least one; its buffer is then as large as that edge needs)
            int i_hi = i_lo + 1;
            while (i_hi < E && off[(size_t)i_hi] < want && off[(size_t)i_hi + 1] - off[(size_t)i_lo] <= slab_records) i_hi++;
            const long long slab_base = off[(size_t)i_lo], cap = std::min<long long>(off[(size_t)i_hi], want) - slab_base;
            if (cap > 0) {
                if (d_rec.n < (size_t)(3 * cap)) { d_rec.free(); d_err.free(); VG_CHECK(d_rec.alloc((size_t)(3 * cap))); VG_CHECK(d_err.alloc((size_t)cap)); }
                const unsigned rb = (unsigned)(((size_t)(i_hi - i_lo) + 3) / 4);
                hipLaunchKernelGGL(k_triplet_records, dim3(rb), dim3(256), 0, st, i_lo, i_hi, d_row.p, d_s0.p, d_s1.p, d_perm.p, d_inv.p, d_R.p, order, d_off.p, slab_base,
                                   cap, d_rec.p, d_err.p);
                VG_CHECK(hipGetLastError());
                VG_CHECK(hipMemcpyAsync(triplet_edges_out + 3 * slab_base, d_rec.p, (size_t)(3 * cap) * sizeof(int), hipMemcpyDeviceToHost, st));
                VG_CHECK(hipMemcpyAsync(triplet_err_out + slab_base, d_err.p, (size_t)cap * sizeof(double), hipMemcpyDeviceToHost, st));
                VG_CHECK(hipStreamSynchronize(st));                                                           // the slab's buffers are reused
            }
            i_lo = i_hi;
        }
    }
    release();
    return SSFM_OK;
}

extern "C" int ssfm_view_graph_tree(int32_t num_cameras, int32_t num_edges, const int32_t* index0, const int32_t* index1, int32_t root, int32_t* num_reached,
                                    int32_t* node_out, int32_t* parent_out, int32_t* edge_out, uint8_t* reversed_out, int32_t* num_levels, int32_t* level_ptr) {
    if (num_edges > 0 && (!index0 || !index1)) return fail(nullptr, SSFM_ERR_INVALID, "ssfm_view_graph_tree: bad arguments");
    if (view_graph_tree(num_cameras, num_edges, index0, index1, root, num_reached, node_out, parent_out, edge_out, reversed_out, num_levels, level_ptr) != 0)
        return fail(nullptr, SSFM_ERR_INVALID, "ssfm_view_graph_tree: root or camera index out of range");
    return SSFM_OK;
}

// ssfm_focal_search with the tree initialisation: see include/ssfm.h.  The host part follows ssfm_focal_search (ransac.hip), except that a failed HIP call gives the temporaries back.
extern "C" int ssfm_focal_search_graph(ssfm_ctx* ctx, int32_t n, int32_t E, const int32_t* index0, const int32_t* index1, const double* rel_rotations,
                                       int32_t inward, double focal_guess, int32_t num_trials, const double* focals, int32_t root, double* costs,
                                       int32_t* best_trial, double* rotations_best, double* rel_rotations_best) {
    const char* who = "ssfm_focal_search_graph";
    if (!ctx || n <= 0 || E <= 0 || num_trials <= 0 || !index0 || !index1 || !rel_rotations || !focals)
        return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": bad arguments");
    if (ctx->collective) return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": the context carries a communicator; this call is single-GPU");
    std::vector<int> t_node((size_t)n), t_parent((size_t)n), t_edge((size_t)n), level_ptr((size_t)n + 1); std::vector<uint8_t> t_rev8((size_t)n);
    int32_t reached = 0, levels = 0;
    if (view_graph_tree(n, E, index0, index1, root, &reached, t_node.data(), t_parent.data(), t_edge.data(), t_rev8.data(), &levels, level_ptr.data()) != 0)
        return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": root or camera index out of range");
    std::vector<int> t_rev(t_rev8.begin(), t_rev8.end());
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // Es[i] = make_spherical_essential_matrix(R_i, inward) (:1429-1433), row-major for the device
    std::vector<double> Es((size_t)9 * E); std::vector<int> e0(index0, index0 + E), e1(index1, index1 + E);
    for (int e = 0; e < E; e++) {
        double Rm[9]; cm_to_rm(rel_rotations + 9 * (size_t)e, Rm);
        double t[3] = {Rm[2], Rm[5], Rm[8] - 1.0}; if (inward) { t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2]; }
        double* Em = &Es[9 * (size_t)e];
        for (int j = 0; j < 3; j++) { Em[j] = t[1] * Rm[6 + j] - t[2] * Rm[3 + j]; Em[3 + j] = t[2] * Rm[j] - t[0] * Rm[6 + j]; Em[6 + j] = t[0] * Rm[3 + j] - t[1] * Rm[j]; }
    }
    DevBuf<double> dEs, dF, dR, dX, dRot, dC; DevBuf<int> de0, de1, dlv, dtn, dtp, dte, dtr;
    auto release = [&]() { dEs.free(); dF.free(); dR.free(); dX.free(); dRot.free(); dC.free(); de0.free(); de1.free(); dlv.free(); dtn.free(); dtp.free(); dte.free(); dtr.free(); };
    std::vector<double> fv(focals, focals + num_trials);
    VG_CHECK(upload(dEs, Es, st)); VG_CHECK(upload(dF, fv, st)); VG_CHECK(upload(de0, e0, st)); VG_CHECK(upload(de1, e1, st));
    VG_CHECK(upload(dlv, level_ptr, st)); VG_CHECK(upload(dtn, t_node, st)); VG_CHECK(upload(dtp, t_parent, st));
    VG_CHECK(upload(dte, t_edge, st)); VG_CHECK(upload(dtr, t_rev, st));
    VG_CHECK(dR.alloc((size_t)num_trials * E * 3)); VG_CHECK(dX.alloc((size_t)num_trials * n * 3));
    VG_CHECK(dRot.alloc((size_t)num_trials * n * 9)); VG_CHECK(dC.alloc(num_trials));
    hipLaunchKernelGGL(k_focal_trials_graph, dim3(num_trials), dim3(256), 0, st, n, E, de0.p, de1.p, levels, dlv.p, dtn.p, dtp.p, dte.p, dtr.p, dEs.p, inward, focal_guess,
                       dF.p, dR.p, dX.p, dRot.p, dC.p);
    VG_CHECK(hipGetLastError());
    std::vector<double> hc(num_trials);
    VG_CHECK(hipMemcpyAsync(hc.data(), dC.p, hc.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    VG_CHECK(hipStreamSynchronize(st));
    int best = 0; for (int t = 1; t < num_trials; t++) if (hc[t] < hc[best]) best = t;                 // :1467-1474 (strict <, first minimum)
    if (costs) std::memcpy(costs, hc.data(), hc.size() * sizeof(double));
    if (best_trial) *best_trial = best;
    if (rotations_best) {
        std::vector<double> hr((size_t)n * 9);
        VG_CHECK(hipMemcpyAsync(hr.data(), dRot.p + (size_t)best * n * 9, hr.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        VG_CHECK(hipStreamSynchronize(st));
        for (int i = 0; i < n; i++) rm_to_cm(&hr[9 * (size_t)i], rotations_best + 9 * (size_t)i);
    }
    if (rel_rotations_best) {                              // the matches as transform_image_matches leaves them at the best focal
        std::vector<double> hr((size_t)E * 3);
        VG_CHECK(hipMemcpyAsync(hr.data(), dR.p + (size_t)best * E * 3, hr.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        VG_CHECK(hipStreamSynchronize(st));
        for (int e = 0; e < E; e++) { double Rm[9]; so3exp(&hr[3 * (size_t)e], Rm); rm_to_cm(Rm, rel_rotations_best + 9 * (size_t)e); }
    }
    release();
    return SSFM_OK;
}
