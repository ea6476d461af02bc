// spherical_sfm_amd -- stereo panorama synthesis: the column loop of make_stereo_panoramas (examples/stereo_panorama_tools.cpp:521-616) with
// synthesize_column_flowbased / synthesize_column_linear (:108-188) as one kernel over the output.  The contract is in include/ssfm.h, the plan in pano_host.h.
//
// The reference walks pair -> thetanum -> phinum and remaps one column of `height` pixels at a time, overwriting columns that a later pair claims again.  Here
// ownership is decided first, on the host (pano_plan: the ok job of the highest pair index), so every output pixel is computed once and no store races.
//
//   k_pano_columns   grid (pano_width / 64, height / 64, num_phi), 256 threads.  A lane owns one output column of one panorama; the 64 lanes of a wave are 64
//                    consecutive columns, which are consecutive thetanum of (nearly always) one pair: they read neighbouring source pixels and store 192
//                    consecutive bytes per row.  A lane per row instead would send the 64 gathers of an instruction to 64 different image rows.  The four waves
//                    of a workgroup interleave the 64 rows of its tile (wave w takes rows w, w + 4, ...), so the vertical taps of one wave are the rows of the
//                    next.  Per lane and tile: the column's record (alpha, tan(phi), synth_R) and the two poses, 33 doubles of y-independent products in
//                    registers; per row: the map in double (pano_host.h's order, four divisions), then fp32: two flow gathers, two frame gathers of four taps
//                    times three bytes (every tap loaded unconditionally from a clamped address, see the samplers), the blend, round half to even, three
//                    byte stores.  First measurement: profiles/pano_notes.md.
//                    A column nobody owns is stored as zeros.  In host-pointer mode the kernel runs once per slab of pairs and touches only the columns whose
//                    owner lies in the slab (the first launch also writes the zeros).
// This unit is compiled with -ffp-contract=off: tests/_pano_ref.py restates the pixel path operation by operation in numpy, which never fuses.
#include <algorithm>
#include <cstring>
#include <thread>
#include "dev_buf.h"
#include "pano_host.h"

namespace ssfm {

constexpr int kPanoLanes = 64;          // columns per workgroup (one wave wide)
constexpr int kPanoWaves = 4;
constexpr int kPanoRows = 64;           // rows per workgroup: 16 per wave
constexpr size_t kPanoPinChunk = (size_t)16 << 20;

struct PanoColDev { double alpha, tan_phi, synth_R[9]; int32_t pair, reserved; };       // one per output column of every panorama; pair < 0: nobody owns it

struct PanoKernelArgs {
    const PanoColDev* cols; const double* R; const double* t;
    const uint8_t* const* frames; const float* const* flow_fwd; const float* const* flow_bwd;     // indexed by frame / by pair; flow_fwd == nullptr: linear mode
    uint8_t* out;
    double focal, cx, cy, synth_focal, depth, synth_radius;
    int32_t n, width, height, pano_width, snap, pair_lo, pair_hi, zero_unowned;
};

// a coordinate that can be sampled: finite and within +-2^30 (false for NaN); then, with snap, moved to the 1/32 grid
__device__ __forceinline__ bool pano_coord(float& x, float& y, int snap) {
    const bool ok = fabsf(x) <= 1073741824.f && fabsf(y) <= 1073741824.f;
    if (snap) { x = rintf(x * 32.f) * 0.03125f; y = rintf(y * 32.f) * 0.03125f; }
    return ok;
}

struct PanoTaps { int ix, iy; float w00, w01, w10, w11; bool x0, x1, y0, y1; };

__device__ __forceinline__ PanoTaps pano_taps(float x, float y, bool ok, int width, int height) {
    PanoTaps T;
    const float xf = floorf(x), yf = floorf(y), fx = x - xf, fy = y - yf;
    T.ix = ok ? (int)xf : -2; T.iy = ok ? (int)yf : -2;
    T.w00 = (1.f - fy) * (1.f - fx); T.w01 = (1.f - fy) * fx; T.w10 = fy * (1.f - fx); T.w11 = fy * fx;
    T.x0 = ok & ((unsigned)T.ix < (unsigned)width); T.x1 = ok & ((unsigned)(T.ix + 1) < (unsigned)width);
    T.y0 = (unsigned)T.iy < (unsigned)height; T.y1 = (unsigned)(T.iy + 1) < (unsigned)height;
    return T;
}

__device__ __forceinline__ float pano_mix(const PanoTaps& T, float t00, float t01, float t10, float t11) {
    return ((t00 * T.w00 + t01 * T.w01) + t10 * T.w10) + t11 * T.w11;
}

// Both samplers load all their taps unconditionally, from clamped and therefore valid addresses, and select afterwards: a load under a lane condition is a branch
// with its own wait, and 32 of them in a row made every row of a wave 32 memory round trips; like this the taps of a sample, and of the two samples of a
// stage, are in flight together.  A tap outside the image enters the sum as 0; a coordinate that cannot be sampled gives 0 whatever its weights are.

// bilinear sample of a two-channel float image
__device__ __forceinline__ void pano_sample_flow(const float* __restrict__ img, int width, int height, float x, float y, int snap, float& ox, float& oy) {
    const bool ok = pano_coord(x, y, snap);
    const PanoTaps T = pano_taps(x, y, ok, width, height);
    const float2* p = reinterpret_cast<const float2*>(img);
    const size_t r0 = (size_t)(T.y0 ? T.iy : 0) * (size_t)width, r1 = (size_t)(T.y1 ? T.iy + 1 : 0) * (size_t)width;
    const size_t c0 = (size_t)(T.x0 ? T.ix : 0), c1 = (size_t)(T.x1 ? T.ix + 1 : 0);
    const float2 l00 = p[r0 + c0], l01 = p[r0 + c1], l10 = p[r1 + c0], l11 = p[r1 + c1];
    const bool b00 = T.y0 & T.x0, b01 = T.y0 & T.x1, b10 = T.y1 & T.x0, b11 = T.y1 & T.x1;
    const float vx = pano_mix(T, b00 ? l00.x : 0.f, b01 ? l01.x : 0.f, b10 ? l10.x : 0.f, b11 ? l11.x : 0.f);
    const float vy = pano_mix(T, b00 ? l00.y : 0.f, b01 ? l01.y : 0.f, b10 ? l10.y : 0.f, b11 ? l11.y : 0.f);
    ox = ok ? vx : 0.f; oy = ok ? vy : 0.f;
}

// bilinear sample of a three-channel byte image
__device__ __forceinline__ void pano_sample_frame(const uint8_t* __restrict__ img, int width, int height, float x, float y, int snap, float* o) {
    const bool ok = pano_coord(x, y, snap);
    const PanoTaps T = pano_taps(x, y, ok, width, height);
    const size_t r0 = (size_t)(T.y0 ? T.iy : 0) * (size_t)width, r1 = (size_t)(T.y1 ? T.iy + 1 : 0) * (size_t)width;
    const size_t c0 = (size_t)(T.x0 ? T.ix : 0), c1 = (size_t)(T.x1 ? T.ix + 1 : 0);
    const uint8_t *p00 = img + (r0 + c0) * 3, *p01 = img + (r0 + c1) * 3, *p10 = img + (r1 + c0) * 3, *p11 = img + (r1 + c1) * 3;
    const bool b00 = T.y0 & T.x0, b01 = T.y0 & T.x1, b10 = T.y1 & T.x0, b11 = T.y1 & T.x1;
    uint8_t l00[3], l01[3], l10[3], l11[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { l00[c] = p00[c]; l01[c] = p01[c]; l10[c] = p10[c]; l11[c] = p11[c]; }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float v = pano_mix(T, b00 ? (float)l00[c] : 0.f, b01 ? (float)l01[c] : 0.f, b10 ? (float)l10[c] : 0.f, b11 ? (float)l11[c] : 0.f);
        o[c] = ok ? v : 0.f;
    }
}

__device__ __forceinline__ uint8_t pano_to_byte(float v) {            // convertTo(CV_8UC3): round half to even, saturate; NaN -> 0
    const float r = rintf(v);
    return (uint8_t)(!(r > 0.f) ? 0.f : r > 255.f ? 255.f : r);
}

__global__ void __launch_bounds__(kPanoLanes * kPanoWaves)
k_pano_columns(const PanoKernelArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * kPanoLanes + lane, phi = blockIdx.z, row0 = blockIdx.y * kPanoRows + wave;
    if (col >= A.pano_width) return;
    const PanoColDev* rec = A.cols + (size_t)phi * (size_t)A.pano_width + (size_t)col;
    const int pair = rec->pair;
    uint8_t* out = A.out + ((size_t)phi * (size_t)A.height * (size_t)A.pano_width + (size_t)col) * 3;
    const size_t out_row = (size_t)A.pano_width * 3;
    if (pair < 0) {
        if (A.zero_unowned)
            for (int y = row0; y < min(row0 + kPanoRows - wave, A.height); y += kPanoWaves) { uint8_t* o = out + (size_t)y * out_row; o[0] = 0; o[1] = 0; o[2] = 0; }
        return;
    }
    if (pair < A.pair_lo || pair >= A.pair_hi) return;
    const int fl = pair, fr = pair + 1 == A.n ? 0 : pair + 1;
    double sR[9], RL[9], RR[9], tL[3], tR[3];
#pragma unroll
    for (int i = 0; i < 9; i++) { sR[i] = rec->synth_R[i]; RL[i] = A.R[(size_t)fl * 9 + i]; RR[i] = A.R[(size_t)fr * 9 + i]; }
#pragma unroll
    for (int i = 0; i < 3; i++) { tL[i] = A.t[(size_t)fl * 3 + i]; tR[i] = A.t[(size_t)fr * 3 + i]; }
    const PanoRowConsts C = pano_row_consts(rec->tan_phi, sR, A.depth, A.synth_radius);
    const double alpha = rec->alpha;
    const float a1 = (float)alpha, a0 = (float)(1.0 - alpha);
    const uint8_t* __restrict__ imgL = A.frames[fl];
    const uint8_t* __restrict__ imgR = A.frames[fr];
    const bool flow = A.flow_fwd != nullptr;
    const float* __restrict__ ff = flow ? A.flow_fwd[pair] : nullptr;
    const float* __restrict__ fb = flow ? A.flow_bwd[pair] : nullptr;
    const int W = A.width, H = A.height, snap = A.snap;
    for (int y = row0; y < min(row0 + kPanoRows - wave, H); y += kPanoWaves) {
        double w[3], XL[3], XR[3];
        pano_world(C, (double)y, A.cy, A.synth_focal, A.depth, w);
        pano_camera(RL, tL, w, XL); pano_camera(RR, tR, w, XR);
        const float xLx = (float)((A.focal * XL[0]) / XL[2] + A.cx), xLy = (float)((A.focal * XL[1]) / XL[2] + A.cy);
        const float xRx = (float)((A.focal * XR[0]) / XR[2] + A.cx), xRy = (float)((A.focal * XR[1]) / XR[2] + A.cy);
        float sLx = xLx, sLy = xLy, sRx = xRx, sRy = xRy;
        if (flow) {
            float fx, fy, gx, gy;
            pano_sample_flow(ff, W, H, xLx, xLy, snap, fx, fy);
            pano_sample_flow(fb, W, H, xRx, xRy, snap, gx, gy);
            const float FsLRx = (xRx - xLx) - fx, FsLRy = (xRy - xLy) - fy, FsRLx = (xLx - xRx) - gx, FsRLy = (xLy - xRy) - gy;
            sLx = xLx * 1.f + FsLRx * a1; sLy = xLy * 1.f + FsLRy * a1;
            sRx = xRx * 1.f + FsRLx * a0; sRy = xRy * 1.f + FsRLy * a0;
        }
        float IL[3], IR[3];
        pano_sample_frame(imgL, W, H, sLx, sLy, snap, IL);
        pano_sample_frame(imgR, W, H, sRx, sRy, snap, IR);
        uint8_t* o = out + (size_t)y * out_row;
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] = pano_to_byte(IL[c] * a0 + IR[c] * a1);
    }
}

// Host memory <-> device through two pinned chunks of the context: the copy of one chunk runs while the host fills (or empties) the other.
struct PanoPipe {
    ssfm_ctx* ctx; hipStream_t st; hipEvent_t ev[2] = {nullptr, nullptr}; bool busy[2] = {false, false}; int turn = 0;
    PanoPipe(ssfm_ctx* c, hipStream_t s) : ctx(c), st(s) {}
    hipError_t init() {
        if (!ctx->pano_pin) {
            if (hipHostMalloc(&ctx->pano_pin, 2 * kPanoPinChunk, hipHostMallocDefault) == hipSuccess) ctx->pano_pin_bytes = 2 * kPanoPinChunk;
            else { ctx->pano_pin = nullptr; ctx->pano_pin_bytes = 0; (void)hipGetLastError(); }             // no pinned memory: plain copies
        }
        for (int i = 0; i < 2; i++) { hipError_t e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
    void destroy() { for (int i = 0; i < 2; i++) { if (ev[i]) (void)hipEventDestroy(ev[i]); ev[i] = nullptr; } }
    char* chunk(int i) const { return static_cast<char*>(ctx->pano_pin) + (size_t)i * kPanoPinChunk; }
    hipError_t h2d(void* dst, const void* src, size_t bytes) {
        if (!ctx->pano_pin) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
        for (size_t off = 0; off < bytes; off += kPanoPinChunk) {
            const size_t len = std::min(kPanoPinChunk, bytes - off);
            if (busy[turn]) { hipError_t e = hipEventSynchronize(ev[turn]); if (e != hipSuccess) return e; }
            std::memcpy(chunk(turn), static_cast<const char*>(src) + off, len);
            hipError_t e = hipMemcpyAsync(static_cast<char*>(dst) + off, chunk(turn), len, hipMemcpyHostToDevice, st); if (e != hipSuccess) return e;
            e = hipEventRecord(ev[turn], st); if (e != hipSuccess) return e;
            busy[turn] = true; turn ^= 1;
        }
        return hipSuccess;
    }
    hipError_t d2h(void* dst, const void* src, size_t bytes) {
        if (!ctx->pano_pin) { hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); return e != hipSuccess ? e : hipStreamSynchronize(st); }
        for (int i = 0; i < 2; i++) if (busy[i]) { hipError_t e = hipEventSynchronize(ev[i]); if (e != hipSuccess) return e; busy[i] = false; }
        size_t prev_off = 0, prev_len = 0; int prev = -1;
        for (size_t off = 0; off < bytes; off += kPanoPinChunk) {
            const size_t len = std::min(kPanoPinChunk, bytes - off);
            hipError_t e = hipMemcpyAsync(chunk(turn), static_cast<const char*>(src) + off, len, hipMemcpyDeviceToHost, st); if (e != hipSuccess) return e;
            e = hipEventRecord(ev[turn], st); if (e != hipSuccess) return e;
            if (prev >= 0) { e = hipEventSynchronize(ev[prev]); if (e != hipSuccess) return e; std::memcpy(static_cast<char*>(dst) + prev_off, chunk(prev), prev_len); }
            prev = turn; prev_off = off; prev_len = len; turn ^= 1;
        }
        if (prev >= 0) { hipError_t e = hipEventSynchronize(ev[prev]); if (e != hipSuccess) return e; std::memcpy(static_cast<char*>(dst) + prev_off, chunk(prev), prev_len); }
        return hipSuccess;
    }
};

static PanoParams pano_params(const ssfm_pano_options* o) {
    PanoParams P;
    if (o) { P.num_phi = o->num_phi; P.phi_step_deg = o->phi_step_deg; P.depth = o->depth; P.synth_radius = o->synth_radius; P.synth_focal_factor = o->synth_focal_factor; P.is_loop = o->is_loop; }
    return P;
}
static int pano_threads() { const unsigned h = std::thread::hardware_concurrency(); return (int)std::min(16u, std::max(1u, h)); }

}  // namespace ssfm
using namespace ssfm;

#define PANO_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipStreamSynchronize(st); release(); return fail(ctx, SSFM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)

extern "C" void ssfm_pano_default_options(ssfm_pano_options* o) {
    if (!o) return;
    o->num_phi = 9; o->is_loop = 1; o->phi_step_deg = 1.0; o->depth = 10.0; o->synth_radius = 0.5; o->synth_focal_factor = 1.2;
    o->subpixel_bits = 0; o->on_device = 0; o->max_slab_bytes = 0;
}

extern "C" int ssfm_pano_last_kernel_ms(ssfm_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SSFM_ERR_INVALID;
    *ms = ctx->pano_kernel_ms;
    return SSFM_OK;
}

extern "C" int ssfm_pano_plan(const ssfm_pano_options* opt, int32_t n, const double* R, const double* t, double focal, double cx, double cy,
                              int32_t width, int32_t height, int32_t pano_width, int32_t* num_jobs, int32_t* job_pair, int32_t* job_theta, int32_t* job_phi,
                              int32_t* job_col, uint8_t* job_ok, double* job_alpha, double* job_consts, int32_t* owner) {
    const char* who = "ssfm_pano_plan";
    (void)cx;
    const PanoParams P = pano_params(opt);
    if (const char* why = pano_check_params(P, n, R, t, focal, width, height, pano_width)) return fail(nullptr, SSFM_ERR_INVALID, std::string(who) + ": " + why);
    if (!num_jobs) return fail(nullptr, SSFM_ERR_INVALID, std::string(who) + ": num_jobs is null");
    PanoPlan plan;
    pano_plan(P, n, R, t, focal, cy, height, pano_width, pano_threads(), plan);
    if (plan.jobs.size() > (size_t)0x7FFFFFFF) return fail(nullptr, SSFM_ERR_INVALID, std::string(who) + ": too many jobs");
    if (owner) std::copy(plan.owner.begin(), plan.owner.end(), owner);
    const int32_t cap = *num_jobs, count = (int32_t)plan.jobs.size();
    *num_jobs = count;
    if (cap < count) return fail(nullptr, SSFM_ERR_INVALID, std::string(who) + ": capacity " + std::to_string(cap) + " is below the " + std::to_string(count) + " jobs of the plan");
    for (int32_t j = 0; j < count; j++) {
        const PanoJob& J = plan.jobs[(size_t)j];
        if (job_pair) job_pair[j] = J.pair;
        if (job_theta) job_theta[j] = J.theta;
        if (job_phi) job_phi[j] = J.phi;
        if (job_col) job_col[j] = J.col;
        if (job_ok) job_ok[j] = J.ok;
        if (job_alpha) job_alpha[j] = J.alpha;
        if (job_consts) { job_consts[(size_t)j * 10] = J.tan_phi; for (int i = 0; i < 9; i++) job_consts[(size_t)j * 10 + 1 + i] = J.synth_R[i]; }
    }
    return SSFM_OK;
}

extern "C" int ssfm_pano_synthesize(ssfm_ctx* ctx, const ssfm_pano_options* opt, int32_t n, const double* R, const double* t, double focal, double cx, double cy,
                                    int32_t width, int32_t height, const uint8_t* const* frames, const float* const* flow_fwd, const float* const* flow_bwd,
                                    int32_t pano_width, uint8_t* panoramas, int32_t* owner_out) {
    const char* who = "ssfm_pano_synthesize";
    auto invalid = [&](const std::string& why) { return fail(ctx, SSFM_ERR_INVALID, std::string(who) + ": " + why); };
    const PanoParams P = pano_params(opt);
    if (const char* why = pano_check_params(P, n, R, t, focal, width, height, pano_width)) return invalid(why);
    if ((flow_fwd == nullptr) != (flow_bwd == nullptr)) return invalid("flow_fwd and flow_bwd must be given together");
    if (!panoramas) return invalid("panoramas is null");
    if (n > 0 && !frames) return invalid("frames is null");
    if (!std::isfinite(cx) || !std::isfinite(cy)) return invalid("cx or cy is not finite");
    const int subpixel = opt ? opt->subpixel_bits : 0, on_device = opt ? opt->on_device : 0;
    if (subpixel != 0 && subpixel != 5) return invalid("subpixel_bits must be 0 or 5");
    if (opt && opt->max_slab_bytes < 0) return invalid("max_slab_bytes is negative");
    const int pairs = pano_num_pairs(n, P.is_loop);
    const bool flow = flow_fwd != nullptr;
    for (int f = 0; f < n; f++) if (!frames[f]) return invalid("frame " + std::to_string(f) + " is null");
    if (flow) for (int k = 0; k < pairs; k++) if (!flow_fwd[k] || !flow_bwd[k]) return invalid("flow of pair " + std::to_string(k) + " is null");
    if (!ctx) return invalid("ctx is null");
    if (ctx->collective) return invalid("the context carries a communicator; this call is single-GPU");
    ctx->pano_kernel_ms = 0.0;

    PanoPlan plan;
    pano_plan(P, n, R, t, focal, cy, height, pano_width, pano_threads(), plan);
    if (owner_out) std::copy(plan.owner.begin(), plan.owner.end(), owner_out);
    const size_t ncols = (size_t)P.num_phi * (size_t)pano_width;
    std::vector<PanoColDev> cols(ncols);
    std::vector<int> owned((size_t)std::max(pairs, 1), 0);
    for (size_t c = 0; c < ncols; c++) {
        PanoColDev& D = cols[c];
        const int32_t j = plan.owner_job[c];
        if (j < 0) { D.alpha = 0.0; D.tan_phi = 0.0; for (int i = 0; i < 9; i++) D.synth_R[i] = 0.0; D.pair = -1; D.reserved = 0; continue; }
        const PanoJob& J = plan.jobs[(size_t)j];
        D.alpha = J.alpha; D.tan_phi = J.tan_phi; for (int i = 0; i < 9; i++) D.synth_R[i] = J.synth_R[i];
        D.pair = J.pair; D.reserved = 0; owned[(size_t)J.pair]++;
    }
    const size_t frame_bytes = (size_t)height * (size_t)width * 3, flow_bytes = (size_t)height * (size_t)width * 2 * sizeof(float);
    const size_t frame_slot = (frame_bytes + 255) / 256 * 256, flow_slot = (flow_bytes + 255) / 256 * 256, out_bytes = ncols * (size_t)height * 3;

    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<PanoColDev> d_cols; DevBuf<double> d_R, d_t; DevBuf<const uint8_t*> d_frames; DevBuf<const float*> d_ff, d_fb; DevBuf<uint8_t> d_slab, d_out;
    std::vector<hipEvent_t> events; PanoPipe pipe(ctx, st);
    auto release = [&]() {
        d_cols.free(); d_R.free(); d_t.free(); d_frames.free(); d_ff.free(); d_fb.free(); d_slab.free(); d_out.free();
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        events.clear(); pipe.destroy();
    };
    std::vector<double> hR(R, R + 9 * (size_t)n), ht(t, t + 3 * (size_t)n);
    PANO_CHECK(upload(d_cols, cols, st)); PANO_CHECK(upload(d_R, hR, st)); PANO_CHECK(upload(d_t, ht, st));
    PANO_CHECK(d_frames.alloc((size_t)n)); PANO_CHECK(d_ff.alloc((size_t)n)); PANO_CHECK(d_fb.alloc((size_t)n));

    PanoKernelArgs A;
    A.cols = d_cols.p; A.R = d_R.p; A.t = d_t.p; A.frames = d_frames.p; A.flow_fwd = flow ? d_ff.p : nullptr; A.flow_bwd = flow ? d_fb.p : nullptr;
    A.focal = focal; A.cx = cx; A.cy = cy; A.synth_focal = focal * P.synth_focal_factor; A.depth = P.depth; A.synth_radius = P.synth_radius;
    A.n = n; A.width = width; A.height = height; A.pano_width = pano_width; A.snap = subpixel == 5 ? 1 : 0;
    const dim3 grid((unsigned)((pano_width + kPanoLanes - 1) / kPanoLanes), (unsigned)((height + kPanoRows - 1) / kPanoRows), (unsigned)P.num_phi);
    auto launch = [&](int k0, int k1, bool first) -> hipError_t {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        hipError_t e = hipEventCreate(&e0); if (e != hipSuccess) return e;
        events.push_back(e0);
        e = hipEventCreate(&e1); if (e != hipSuccess) return e;
        events.push_back(e1);
        A.pair_lo = k0; A.pair_hi = k1; A.zero_unowned = first ? 1 : 0;
        e = hipEventRecord(e0, st); if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_pano_columns, grid, dim3(kPanoLanes * kPanoWaves), 0, st, A);
        e = hipGetLastError(); if (e != hipSuccess) return e;
        return hipEventRecord(e1, st);
    };

    if (on_device) {
        A.out = panoramas;
        if (n > 0) {
            PANO_CHECK(hipMemcpyAsync(d_frames.p, frames, (size_t)n * sizeof(void*), hipMemcpyHostToDevice, st));
            if (flow) {
                PANO_CHECK(hipMemcpyAsync(d_ff.p, flow_fwd, (size_t)pairs * sizeof(void*), hipMemcpyHostToDevice, st));
                PANO_CHECK(hipMemcpyAsync(d_fb.p, flow_bwd, (size_t)pairs * sizeof(void*), hipMemcpyHostToDevice, st));
            }
        }
        PANO_CHECK(launch(0, pairs, true));
    } else {
        PANO_CHECK(d_out.alloc(out_bytes));
        A.out = d_out.p;
        PANO_CHECK(pipe.init());
        // pairs per slab: m pairs hold m + 1 frames and, in flow mode, 2 m flow fields
        const size_t budget = opt && opt->max_slab_bytes > 0 ? (size_t)opt->max_slab_bytes : (size_t)1 << 30;
        const size_t per_pair = frame_slot + (flow ? 2 * flow_slot : 0);
        size_t m = budget > frame_slot ? (budget - frame_slot) / per_pair : 0;
        m = std::max<size_t>(1, std::min<size_t>(m, (size_t)std::max(pairs, 1)));
        PANO_CHECK(d_slab.alloc(frame_slot * (m + 1) + (flow ? 2 * flow_slot * m : 0)));
        std::vector<const uint8_t*> tf((size_t)std::max(n, 1)); std::vector<const float*> tff((size_t)std::max(n, 1)), tfb((size_t)std::max(n, 1));
        bool first = true;
        for (int k0 = 0; k0 < pairs; k0 += (int)m) {
            const int k1 = std::min(pairs, k0 + (int)m);
            if (!std::any_of(owned.begin() + k0, owned.begin() + k1, [](int c) { return c > 0; })) continue;      // nothing of this slab reaches the output
            // the pointer tables and the slab are read by the previous launch: wait for it before the host rewrites the tables' source
            PANO_CHECK(hipStreamSynchronize(st));
            std::fill(tf.begin(), tf.end(), nullptr); std::fill(tff.begin(), tff.end(), nullptr); std::fill(tfb.begin(), tfb.end(), nullptr);
            uint8_t* base = d_slab.p;
            for (int s = 0; s <= k1 - k0; s++) {                       // frame slot s holds frame (k0 + s) mod n, uploaded when a pair with columns reads it
                const int f = (k0 + s) % n;
                const bool need = (s < k1 - k0 && owned[(size_t)(k0 + s)] > 0) || (s > 0 && owned[(size_t)(k0 + s - 1)] > 0);
                if (!need || tf[(size_t)f]) continue;                  // (a loop's last slot is frame 0 again)
                uint8_t* dst = base + frame_slot * (size_t)s;
                PANO_CHECK(pipe.h2d(dst, frames[f], frame_bytes));
                tf[(size_t)f] = dst;
            }
            if (flow) {
                uint8_t* fbase = base + frame_slot * (m + 1);
                for (int s = 0; s < k1 - k0; s++) {
                    if (owned[(size_t)(k0 + s)] == 0) continue;
                    uint8_t* d0 = fbase + flow_slot * (size_t)(2 * s), *d1 = d0 + flow_slot;
                    PANO_CHECK(pipe.h2d(d0, flow_fwd[k0 + s], flow_bytes)); PANO_CHECK(pipe.h2d(d1, flow_bwd[k0 + s], flow_bytes));
                    tff[(size_t)(k0 + s)] = reinterpret_cast<const float*>(d0); tfb[(size_t)(k0 + s)] = reinterpret_cast<const float*>(d1);
                }
            }
            PANO_CHECK(hipMemcpyAsync(d_frames.p, tf.data(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, st));
            if (flow) {
                PANO_CHECK(hipMemcpyAsync(d_ff.p, tff.data(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, st));
                PANO_CHECK(hipMemcpyAsync(d_fb.p, tfb.data(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, st));
            }
            PANO_CHECK(hipStreamSynchronize(st));                      // the tables are pageable host memory: copied before they change again
            PANO_CHECK(launch(k0, k1, first));
            first = false;
        }
        if (first) PANO_CHECK(launch(0, 0, true));                     // no pair owns a column: the zeros are still written
        PANO_CHECK(pipe.d2h(panoramas, d_out.p, out_bytes));
    }
    PANO_CHECK(hipStreamSynchronize(st));
    double total = 0.0;
    for (size_t i = 0; i + 1 < events.size(); i += 2) { float ms = 0.f; if (hipEventElapsedTime(&ms, events[i], events[i + 1]) == hipSuccess) total += ms; else (void)hipGetLastError(); }
    ctx->pano_kernel_ms = total;
    release();
    return SSFM_OK;
}
