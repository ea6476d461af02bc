// spherical_sfm_amd -- robust rotation initialisation over a view graph: L1 iteratively reweighted least squares (include/ssfm.h: ssfm_rot_l1_init).
//
// One outer iteration is a weighted graph Laplacian with three right-hand sides, solved by Jacobi-preconditioned conjugate gradients that stay on the device:
//   k_l1_edges      a lane per edge: v_e = so3ln(R_b^T R_e R_a), w_e = 1 / max(|v_e|, floor), the record (w, w v); per-workgroup partials of sum |v_e|
//   k_l1_nodes      a wave per node over the node-major adjacency of rot_l1_host.h: L_ii, g_i and the CG start x = 0, r = g, z = r / L_ii, p = z;
//                   per-workgroup partials of r.z and g.g per column
//   k_l1_matvec     a wave per node: q_i = L_ii p_i - sum w_e p_nb(e) by gathers; per-workgroup partials of p.q per column
//   k_l1_cg_update  one workgroup strided over 3 n: folds the partials, alpha and beta per column, x, r, z, p, the column flags, the iteration counter, the done word
//   k_l1_apply      a lane per node: R_i <- R_i so3exp(x_i); per-workgroup maxima of |x_i|
// The host enqueues CG iterations in chunks of kChunk (matvec + update; both return at once when the done word is set) and reads the done word and the
// counters through the context's pinned staging after each chunk, the step once per outer iteration.  alpha, beta and the flags never leave the device.
// The root and every camera it does not reach are rows of the vectors like any other, with x = r = p = q = 0 and L_ii = 1: the gathers then see x_root = 0 and
// the system the free nodes solve is the reduced Laplacian.
//
// REPRODUCIBLE: there is no floating-point atomic in this file.  A lane adds its strided share in ascending order, a wave folds by the xor butterfly (wave_sum),
// a workgroup adds its waves in wave order, the update adds the workgroups' partials in workgroup order and folds its own lanes by a fixed halving tree.  Two
// calls on the same input return the same bits.
#include <algorithm>
#include <cstring>
#include "ba_flatten.h"
#include "ba_kernels.h"
#include "dev_buf.h"
#include "rot_l1_host.h"

namespace ssfm {

enum { L1_FLAG = 0, L1_ITERS = 3, L1_DONE = 4, L1_CAPPED = 5, L1_ISTATE = 8 };     // the int state words
enum { L1_RZ = 0, L1_GG = 3, L1_DSTATE = 8 };                                       // the double state words
static constexpr int kUpdateThreads = 384;                                          // a multiple of 3 and of 64: thread t only ever sees column t % 3

__global__ void __launch_bounds__(256)
k_l1_edges(int E, const int* __restrict__ e0, const int* __restrict__ e1, const int* __restrict__ reached, const double* __restrict__ rel /*[E*9] row-major*/,
           const double* __restrict__ rot /*[n*9] row-major*/, double floor_w, double* __restrict__ rec /*[E*4]*/, double* __restrict__ residual /*[E] or null*/,
           double* __restrict__ cost_part) {
    __shared__ double red[4];
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double nrm = 0.0;
    if (e < E) {
        const int a = e0[e], b = e1[e];
        const bool used = a != b && reached[a] && reached[b];
        double v[3] = {0.0, 0.0, 0.0}, w = 0.0;
        if (used) {
            double Re[9], Ra[9], Rb[9], T[9], D[9];
#pragma unroll
            for (int q = 0; q < 9; q++) { Re[q] = rel[9 * (size_t)e + q]; Ra[q] = rot[9 * (size_t)a + q]; Rb[q] = rot[9 * (size_t)b + q]; }
            mat3_mul(Re, Ra, T); mat3_mul_at(Rb, T, D);
            so3ln(D, v);
            nrm = norm3(v);
            w = 1.0 / fmax(nrm, floor_w);
        }
        double* o = rec + 4 * (size_t)e;
        o[0] = w; o[1] = w * v[0]; o[2] = w * v[1]; o[3] = w * v[2];
        if (residual) residual[e] = used ? nrm : -1.0;
    }
    const double s = wave_sum(nrm);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) cost_part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(256)
k_l1_nodes(int n, const int* __restrict__ free_node, const int* __restrict__ adj_ptr, const unsigned* __restrict__ adj_es, const double* __restrict__ rec,
           double* __restrict__ Lii, double* __restrict__ x, double* __restrict__ r, double* __restrict__ z, double* __restrict__ p, double* __restrict__ q,
           double* __restrict__ part /*[blocks*6]: r.z, g.g per column*/) {
    __shared__ double red[4][6];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + wv;
    const bool fr = i < n && free_node[i] != 0;                                     // wave-uniform
    double sw = 0.0, g[3] = {0.0, 0.0, 0.0};
    if (fr) {
        for (int k = adj_ptr[i] + lane; k < adj_ptr[i + 1]; k += 64) {
            const unsigned es = adj_es[k];
            const double* o = rec + 4 * (size_t)(es >> 1);
            const double sgn = (es & 1u) ? 1.0 : -1.0;
            sw += o[0]; g[0] += sgn * o[1]; g[1] += sgn * o[2]; g[2] += sgn * o[3];
        }
    }
    sw = wave_sum(sw); g[0] = wave_sum(g[0]); g[1] = wave_sum(g[1]); g[2] = wave_sum(g[2]);
    if (lane == 0) {
        const double d = fr ? sw : 1.0;                                             // a free node has an edge to its tree parent: sw > 0
        if (i < n) {
            Lii[i] = d;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double zc = g[c] / d;
                x[3 * i + c] = 0.0; r[3 * i + c] = g[c]; z[3 * i + c] = zc; p[3 * i + c] = zc; q[3 * i + c] = 0.0;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) { red[wv][c] = g[c] * (g[c] / d); red[wv][3 + c] = g[c] * g[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) part[6 * (size_t)blockIdx.x + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ void __launch_bounds__(256)
k_l1_matvec(int n, const int* __restrict__ free_node, const int* __restrict__ adj_ptr, const int* __restrict__ adj_nb, const unsigned* __restrict__ adj_es,
            const double* __restrict__ rec, const double* __restrict__ Lii, const double* __restrict__ p, double* __restrict__ q,
            double* __restrict__ part /*[blocks*3]: p.q per column*/, const int* __restrict__ istate) {
    __shared__ double red[4][3];
    if (istate[L1_DONE]) return;                                                     // grid-uniform
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + wv;
    const bool fr = i < n && free_node[i] != 0;
    double a[3] = {0.0, 0.0, 0.0};
    if (fr) {
        for (int k = adj_ptr[i] + lane; k < adj_ptr[i + 1]; k += 64) {
            const double w = rec[4 * (size_t)(adj_es[k] >> 1)];
            const double* pn = p + 3 * (size_t)adj_nb[k];
            a[0] += w * pn[0]; a[1] += w * pn[1]; a[2] += w * pn[2];
        }
    }
    a[0] = wave_sum(a[0]); a[1] = wave_sum(a[1]); a[2] = wave_sum(a[2]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double pq = 0.0;
            if (fr) { const double pc = p[3 * i + c], qc = Lii[i] * pc - a[c]; q[3 * i + c] = qc; pq = pc * qc; }
            red[wv][c] = pq;
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) part[3 * (size_t)blockIdx.x + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// INIT: fold the partials of k_l1_nodes, set the column flags (the stopping test before the first iteration), clear the counters.
// otherwise: one CG iteration of every column that is not flagged.
template <bool INIT>
__global__ void __launch_bounds__(kUpdateThreads)
k_l1_cg_update(int n3, int nblk, const double* __restrict__ part, double* __restrict__ dstate, int* __restrict__ istate, double tol2, int cap,
               const double* __restrict__ Lii, double* __restrict__ x, double* __restrict__ r, double* __restrict__ z, double* __restrict__ p,
               const double* __restrict__ q) {
    __shared__ double s_a[kUpdateThreads], s_b[kUpdateThreads], s_coef[3];
    __shared__ int s_act[3], s_flag[3];
    const int t = threadIdx.x, c = t % 3;
    if (INIT) {
        if (t < 3) {
            double rz = 0.0, gg = 0.0;
            for (int b = 0; b < nblk; b++) { rz += part[6 * (size_t)b + t]; gg += part[6 * (size_t)b + 3 + t]; }
            dstate[L1_RZ + t] = rz; dstate[L1_GG + t] = gg;
            const int flag = gg <= tol2 * gg ? 1 : 0;                                // r = g: a zero column is done at once
            istate[L1_FLAG + t] = flag; s_flag[t] = flag;
        }
        __syncthreads();
        if (t == 0) {
            const bool all = s_flag[0] && s_flag[1] && s_flag[2];
            istate[L1_ITERS] = 0; istate[L1_DONE] = (all || cap <= 0) ? 1 : 0; istate[L1_CAPPED] = (!all && cap <= 0) ? 1 : 0;
        }
        return;
    }
    if (istate[L1_DONE]) return;                                                     // uniform
    if (t < 3) {
        double pq = 0.0;
        for (int b = 0; b < nblk; b++) pq += part[3 * (size_t)b + t];
        const int act = istate[L1_FLAG + t] ? 0 : 1;
        s_act[t] = act; s_coef[t] = act ? dstate[L1_RZ + t] / pq : 0.0;
    }
    __syncthreads();
    const int act = s_act[c];
    const double alpha = s_coef[c];
    double lrz = 0.0, lrr = 0.0;
    if (act) {
        for (int j = t; j < n3; j += kUpdateThreads) {                               // j % 3 == c for every j of this thread
            const double xj = x[j] + alpha * p[j], rj = r[j] - alpha * q[j], zj = rj / Lii[j / 3];
            x[j] = xj; r[j] = rj; z[j] = zj;
            lrz += rj * zj; lrr += rj * rj;
        }
    }
    s_a[t] = lrz; s_b[t] = lrr;
    __syncthreads();
    for (int h = kUpdateThreads / 6; h >= 1; h >>= 1) {                              // 3 h partners apart keeps the column; 128 lanes per column
        if (t < 3 * h) { s_a[t] += s_a[t + 3 * h]; s_b[t] += s_b[t + 3 * h]; }
        __syncthreads();
    }
    if (t < 3) {
        int flag = 1; double beta = 0.0;
        if (act) {
            const double rz_new = s_a[t], rr = s_b[t];
            beta = rz_new / dstate[L1_RZ + t];
            dstate[L1_RZ + t] = rz_new;
            flag = rr <= tol2 * dstate[L1_GG + t] ? 1 : 0;
            istate[L1_FLAG + t] = flag;
        }
        s_flag[t] = flag; s_coef[t] = beta;
    }
    __syncthreads();
    if (act) {
        const double beta = s_coef[c];
        for (int j = t; j < n3; j += kUpdateThreads) p[j] = z[j] + beta * p[j];
    }
    if (t == 0) {
        const int iters = istate[L1_ITERS] + 1;
        const bool all = s_flag[0] && s_flag[1] && s_flag[2];
        istate[L1_ITERS] = iters; istate[L1_DONE] = (all || iters >= cap) ? 1 : 0; istate[L1_CAPPED] = (!all && iters >= cap) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256)
k_l1_apply(int n, const int* __restrict__ free_node, const double* __restrict__ x, double* __restrict__ rot, double* __restrict__ step_part) {
    __shared__ double red[4];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double m = 0.0;
    if (i < n && free_node[i]) {
        double R[9], dR[9], Rn[9];
        const double xi[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = rot[9 * (size_t)i + k];
        so3exp(xi, dR); mat3_mul(R, dR, Rn);
#pragma unroll
        for (int k = 0; k < 9; k++) rot[9 * (size_t)i + k] = Rn[k];
        m = norm3(xi);
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) step_part[blockIdx.x] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

}  // namespace ssfm
using namespace ssfm;

static const int kChunk = 16;      // CG iterations enqueued between two looks at the done word

extern "C" void ssfm_rot_l1_default_options(ssfm_rot_l1_options* o) {
    if (!o) return;
    o->max_iterations = 30; o->step_tolerance = 1e-4; o->weight_floor = 1e-3; o->pcg_tolerance = 1e-10; o->pcg_max_iterations = 0;
}

// a failed HIP call: wait for what is in flight, give the temporaries back (ssfm_ctx.h: the pool's rule), report
#define L1_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipStreamSynchronize(st); release(); return fail(ctx, SSFM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)

extern "C" int ssfm_rot_l1_init(ssfm_ctx* ctx, int32_t num_cameras, int32_t num_edges, const int32_t* index0, const int32_t* index1, const double* rel_rotations,
                                int32_t root, const ssfm_rot_l1_options* opt, double* rotations_out, double* residual_out, ssfm_rot_l1_summary* s) {
    const std::string who = "ssfm_rot_l1_init: ";
    if (const char* why = rot_l1_check(num_cameras, num_edges, index0, index1, rel_rotations, root, opt, rotations_out, s))
        return fail(ctx, SSFM_ERR_INVALID, who + why);                                                       // before anything is launched
    if (!ctx) return fail(ctx, SSFM_ERR_INVALID, who + "ctx is null");
    if (ctx->collective) return fail(ctx, SSFM_ERR_INVALID, who + "the context carries a communicator; this call is single-GPU");
    ssfm_rot_l1_options O;
    if (opt) O = *opt; else ssfm_rot_l1_default_options(&O);
    const int n = num_cameras, E = num_edges;
    RotL1Graph G;
    if (!rot_l1_graph(n, E, index0, index1, root, G)) return fail(ctx, SSFM_ERR_INVALID, who + "root or camera index out of range");
    std::memset(s, 0, sizeof(*s));
    s->termination = SSFM_CONVERGENCE; s->num_free = G.num_free; s->num_edges_used = G.num_edges_used;
    // the tree start (row-major inside)
    std::vector<double> rel((size_t)9 * E), rot((size_t)9 * n);
    for (int e = 0; e < E; e++) cm_to_rm(rel_rotations + 9 * (size_t)e, &rel[9 * (size_t)e]);
    view_graph_chain(n, G.num_reached, G.t_node.data(), G.t_parent.data(), G.t_edge.data(), G.t_rev.data(), rel.data(), rot.data());
    if (G.num_edges_used == 0) {                                                                             // nothing to solve: identities
        for (int i = 0; i < n; i++) rm_to_cm(&rot[9 * (size_t)i], rotations_out + 9 * (size_t)i);
        if (residual_out) for (int e = 0; e < E; e++) residual_out[e] = -1.0;
        return SSFM_OK;
    }
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const unsigned nb_edges = (unsigned)(((size_t)E + 255) / 256), nb_nodes = (unsigned)(((size_t)n + 3) / 4), nb_apply = (unsigned)(((size_t)n + 255) / 256);
    // pinned staging: the int state (4 doubles), then the cost partials, then the step partials.  Nothing of this context is in flight here, so it may move.
    const size_t stage_need = 4 + (size_t)nb_edges + nb_apply;
    if (ctx->dl_stage_n < stage_need) {
        if (ctx->dl_stage) (void)hipHostFree(ctx->dl_stage);
        ctx->dl_stage = nullptr; ctx->dl_stage_n = 0;
        SSFM_HIP_CHECK(ctx, hipHostMalloc((void**)&ctx->dl_stage, stage_need * sizeof(double), hipHostMallocDefault));
        ctx->dl_stage_n = stage_need;
    }
    int* h_istate = reinterpret_cast<int*>(ctx->dl_stage); double* h_cost = ctx->dl_stage + 4; double* h_step = h_cost + nb_edges;
    std::vector<int> e0(index0, index0 + E), e1(index1, index1 + E);
    DevBuf<int> d_e0, d_e1, d_reached, d_free, d_aptr, d_anb, d_istate; DevBuf<unsigned> d_aes;
    DevBuf<double> d_rel, d_rot, d_rec, d_res, d_cost, d_L, d_x, d_r, d_z, d_p, d_q, d_part, d_dstate, d_step;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    auto release = [&]() {
        d_e0.free(); d_e1.free(); d_reached.free(); d_free.free(); d_aptr.free(); d_anb.free(); d_istate.free(); d_aes.free(); d_rel.free(); d_rot.free(); d_rec.free();
        d_res.free(); d_cost.free(); d_L.free(); d_x.free(); d_r.free(); d_z.free(); d_p.free(); d_q.free(); d_part.free(); d_dstate.free(); d_step.free();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        ev0 = ev1 = nullptr;
    };
    L1_CHECK(hipEventCreate(&ev0)); L1_CHECK(hipEventCreate(&ev1));
    L1_CHECK(upload(d_e0, e0, st)); L1_CHECK(upload(d_e1, e1, st)); L1_CHECK(upload(d_reached, G.reached, st)); L1_CHECK(upload(d_free, G.free_node, st));
    L1_CHECK(upload(d_aptr, G.adj_ptr, st)); L1_CHECK(upload(d_anb, G.adj_nb, st)); L1_CHECK(upload(d_aes, G.adj_es, st));
    L1_CHECK(upload(d_rel, rel, st)); L1_CHECK(upload(d_rot, rot, st));
    L1_CHECK(d_rec.alloc((size_t)4 * E)); L1_CHECK(d_res.alloc(E)); L1_CHECK(d_cost.alloc(nb_edges)); L1_CHECK(d_L.alloc(n));
    L1_CHECK(d_x.alloc((size_t)3 * n)); L1_CHECK(d_r.alloc((size_t)3 * n)); L1_CHECK(d_z.alloc((size_t)3 * n)); L1_CHECK(d_p.alloc((size_t)3 * n));
    L1_CHECK(d_q.alloc((size_t)3 * n)); L1_CHECK(d_part.alloc((size_t)6 * nb_nodes)); L1_CHECK(d_dstate.alloc(L1_DSTATE)); L1_CHECK(d_istate.alloc(L1_ISTATE));
    L1_CHECK(d_step.alloc(nb_apply));
    const int cap = O.pcg_max_iterations > 0 ? O.pcg_max_iterations : (int)std::min<long long>(4LL * G.num_free, 0x7fffffffLL);
    const double tol2 = O.pcg_tolerance * O.pcg_tolerance;
    auto edges_pass = [&](double* residual) {
        hipLaunchKernelGGL(k_l1_edges, dim3(nb_edges), dim3(256), 0, st, E, d_e0.p, d_e1.p, d_reached.p, d_rel.p, d_rot.p, O.weight_floor, d_rec.p, residual, d_cost.p);
    };
    auto host_cost = [&]() { double c = 0.0; for (unsigned b = 0; b < nb_edges; b++) c += h_cost[b]; return c; };
    L1_CHECK(hipEventRecord(ev0, st));
    for (int k = 1; k <= O.max_iterations; k++) {
        edges_pass(nullptr);
        L1_CHECK(hipGetLastError());
        if (k == 1) L1_CHECK(hipMemcpyAsync(h_cost, d_cost.p, nb_edges * sizeof(double), hipMemcpyDeviceToHost, st));   // read with the first chunk's state
        hipLaunchKernelGGL(k_l1_nodes, dim3(nb_nodes), dim3(256), 0, st, n, d_free.p, d_aptr.p, d_aes.p, d_rec.p, d_L.p, d_x.p, d_r.p, d_z.p, d_p.p, d_q.p, d_part.p);
        L1_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_l1_cg_update<true>, dim3(1), dim3(kUpdateThreads), 0, st, 3 * n, (int)nb_nodes, d_part.p, d_dstate.p, d_istate.p, tol2, cap, d_L.p, d_x.p,
                           d_r.p, d_z.p, d_p.p, d_q.p);
        L1_CHECK(hipGetLastError());
        for (;;) {
            for (int c = 0; c < kChunk; c++) {
                hipLaunchKernelGGL(k_l1_matvec, dim3(nb_nodes), dim3(256), 0, st, n, d_free.p, d_aptr.p, d_anb.p, d_aes.p, d_rec.p, d_L.p, d_p.p, d_q.p, d_part.p, d_istate.p);
                hipLaunchKernelGGL(k_l1_cg_update<false>, dim3(1), dim3(kUpdateThreads), 0, st, 3 * n, (int)nb_nodes, d_part.p, d_dstate.p, d_istate.p, tol2, cap, d_L.p,
                                   d_x.p, d_r.p, d_z.p, d_p.p, d_q.p);
            }
            L1_CHECK(hipGetLastError());
            L1_CHECK(hipMemcpyAsync(h_istate, d_istate.p, L1_ISTATE * sizeof(int), hipMemcpyDeviceToHost, st));
            L1_CHECK(hipStreamSynchronize(st));
            if (h_istate[L1_DONE]) break;
        }
        if (k == 1) s->initial_cost = host_cost();
        s->pcg_iterations_total += h_istate[L1_ITERS];
        if (h_istate[L1_CAPPED]) s->pcg_solves_capped++;
        hipLaunchKernelGGL(k_l1_apply, dim3(nb_apply), dim3(256), 0, st, n, d_free.p, d_x.p, d_rot.p, d_step.p);
        L1_CHECK(hipGetLastError());
        L1_CHECK(hipMemcpyAsync(h_step, d_step.p, nb_apply * sizeof(double), hipMemcpyDeviceToHost, st));
        L1_CHECK(hipStreamSynchronize(st));
        double step = 0.0;
        for (unsigned b = 0; b < nb_apply; b++) step = std::max(step, h_step[b]);
        s->iterations = k; s->last_step = step;
        if (step < O.step_tolerance) { s->termination = SSFM_CONVERGENCE; break; }
        s->termination = SSFM_NO_CONVERGENCE;
    }
    edges_pass(d_res.p);                                                                                     // the last pass: residuals at the returned rotations
    L1_CHECK(hipGetLastError());
    L1_CHECK(hipEventRecord(ev1, st));
    std::vector<double> hres((size_t)E);
    L1_CHECK(hipMemcpyAsync(h_cost, d_cost.p, nb_edges * sizeof(double), hipMemcpyDeviceToHost, st));
    L1_CHECK(hipMemcpyAsync(hres.data(), d_res.p, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, st));
    L1_CHECK(hipMemcpyAsync(rot.data(), d_rot.p, rot.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    L1_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    L1_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
    s->kernel_ms = ms; s->final_cost = host_cost();
    for (int i = 0; i < n; i++) rm_to_cm(&rot[9 * (size_t)i], rotations_out + 9 * (size_t)i);
    if (residual_out) std::memcpy(residual_out, hres.data(), (size_t)E * sizeof(double));
    release();                                                                                               // the stream has drained
    return SSFM_OK;
}
