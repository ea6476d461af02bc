// spherical_sfm_amd -- context + communicator entry points of the C ABI (include/ssfm.h).
#include <cstdlib>
#include <cstring>
#include "ssfm_ctx.h"
#include "knobs.h"

namespace ssfm { std::string g_last_error; }
using namespace ssfm;

extern "C" int ssfm_version(void) { return 100; }

extern "C" int ssfm_ctx_create(int32_t device, void* stream, ssfm_ctx** out) {
    if (!out) return fail(nullptr, SSFM_ERR_INVALID, "ssfm_ctx_create: out is null");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail(nullptr, SSFM_ERR_NO_DEVICE, "ssfm_ctx_create: no HIP device (the MI355X path has no CPU fallback)");
    if (device < 0) { e = hipGetDevice(&device); if (e != hipSuccess) return fail(nullptr, SSFM_ERR_HIP, hipGetErrorString(e)); }
    if (device >= count) return fail(nullptr, SSFM_ERR_INVALID, "ssfm_ctx_create: device index out of range");
    e = hipSetDevice(device); if (e != hipSuccess) return fail(nullptr, SSFM_ERR_HIP, hipGetErrorString(e));
    ssfm_ctx* c = new ssfm_ctx();
    c->device = device;
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else {
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete c; return fail(nullptr, SSFM_ERR_HIP, hipGetErrorString(e)); }
        c->own_stream = true;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cus = prop.multiProcessorCount;
    { int lds = 0; if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds >= 64 * 1024) ssfm::plan_lds_limit() = (size_t)lds; }      // what the planners may ask for (ba_flatten.h)
    *out = c;
    return SSFM_OK;
}

void ssfm_host_stash_clear();
extern "C" void ssfm_ctx_destroy(ssfm_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->plan_cache && ctx->plan_cache_free) ctx->plan_cache_free(ctx->plan_cache);
    g_dev_pool.drain(ctx->device);                               // recycled device buffers of this device
    ssfm_host_stash_clear();                                     // recycled host arrays of the planner (ba_solver.hip)
    if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
    if (ctx->host_stage) (void)hipHostFree(ctx->host_stage);
    if (ctx->dl_stage) (void)hipHostFree(ctx->dl_stage);
    if (ctx->host_pub) (void)hipHostFree(ctx->host_pub);
    if (ctx->tracks_dev) (void)hipFree(ctx->tracks_dev);
    if (ctx->tracks_pin) (void)hipHostFree(ctx->tracks_pin);
    if (ctx->pano_pin) (void)hipHostFree(ctx->pano_pin);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" const char* ssfm_last_error(const ssfm_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

extern "C" int ssfm_comm_unique_id(uint8_t id[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId u;
    ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) return fail(nullptr, SSFM_ERR_COMM, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memcpy(id, &u, 128);
    return SSFM_OK;
}

extern "C" int ssfm_comm_init(ssfm_ctx* ctx, const uint8_t id[128], int32_t nranks, int32_t rank) {
    if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, SSFM_ERR_INVALID, "ssfm_comm_init: bad arguments");
    // a 1-rank job needs no communicator; SSFM_COMM_SINGLE_RANK=1 creates one anyway so that the RCCL code path can be
    // exercised on a single GPU (tests)
    const char* force = std::getenv("SSFM_COMM_SINGLE_RANK");
    if (nranks == 1 && !(force && force[0] == '1')) { ctx->nranks = 1; ctx->rank = 0; ctx->collective = false; return SSFM_OK; }
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ncclUniqueId u; std::memcpy(&u, id, 128);
    SSFM_NCCL_CHECK(ctx, ncclCommInitRank(&ctx->comm, nranks, u, rank));
    ctx->nranks = nranks; ctx->rank = rank; ctx->collective = true;
    return SSFM_OK;
}

extern "C" int ssfm_comm_init_host(ssfm_ctx* ctx, int32_t nranks, int32_t rank, ssfm_host_allreduce_fn fn, void* user) {
    if (!ctx || !fn || nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, SSFM_ERR_INVALID, "ssfm_comm_init_host: bad arguments");
    if (ctx->comm) return fail(ctx, SSFM_ERR_INVALID, "ssfm_comm_init_host: an RCCL communicator is already attached");
    ctx->host_allreduce = fn; ctx->host_allreduce_user = user;
    ctx->nranks = nranks; ctx->rank = rank; ctx->collective = true;
    return SSFM_OK;
}

// bench.py's `timing_without_collective` probe (never a product setting): BA reductions of this context return at once while `on` is set
extern "C" int ssfm_debug_timing_skip_collectives(ssfm_ctx* ctx, int32_t on) {
    if (!ctx) return SSFM_ERR_INVALID;
    if (on && !ctx->timing_skip_collectives)
        std::fprintf(stderr, "[ssfm] WARNING: collectives of this context are SKIPPED (timing probe): multi-rank bundle adjustment results are meaningless until it is switched off\n");
    ctx->timing_skip_collectives = on != 0;
    return SSFM_OK;
}

// ---- measured device copy bandwidth: the denominator SURVEY.md 8d asks for next to the nominal 8 TB/s ----
// grid-stride copy of 16-byte words (float4), `bytes` read + `bytes` written per launch; GBs_out = (2 x bytes) / average launch time over `reps` launches
// (hipEvents on the context's stream, after two warm-up launches).  The buffers are larger than the 256 MB Infinity Cache when bytes >= 256 MB.
template <int INFLIGHT>
static __global__ void __launch_bounds__(256) k_copy16(const float4* __restrict__ src, float4* __restrict__ dst, size_t n16) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (INFLIGHT == 4)
        for (; i + 3 * stride < n16; i += 4 * stride) {          // four 16-byte loads in flight per lane before the first store
            const float4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
            dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
        }
    for (; i < n16; i += stride) dst[i] = src[i];
}
// best of a few launch shapes (blocks per CU x loads in flight) and of the runtime's own device-to-device copy: the figure is a property of the box, not of one shape
extern "C" int ssfm_debug_copy_bandwidth(ssfm_ctx* ctx, uint64_t bytes, int32_t reps, double* GBs_out) {
    if (!ctx || !GBs_out || bytes < 4096 || reps < 1) return fail(ctx, SSFM_ERR_INVALID, "ssfm_debug_copy_bandwidth: bad arguments");
    SSFM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t n16 = bytes / 16; float4 *a = nullptr, *b = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
    auto body = [&]() -> int {
        SSFM_HIP_CHECK(ctx, hipMalloc((void**)&a, n16 * 16)); SSFM_HIP_CHECK(ctx, hipMalloc((void**)&b, n16 * 16));
        SSFM_HIP_CHECK(ctx, hipMemsetAsync(a, 1, n16 * 16, ctx->stream)); SSFM_HIP_CHECK(ctx, hipMemsetAsync(b, 0, n16 * 16, ctx->stream));
        SSFM_HIP_CHECK(ctx, hipEventCreate(&e0)); SSFM_HIP_CHECK(ctx, hipEventCreate(&e1));
        double best = 0.0;
        for (int shape = 0; shape < 9; shape++) {
            const int per_cu[4] = {8, 16, 32, 64}; const int grid = ctx->num_cus * per_cu[shape % 4]; const bool four = shape >= 4 && shape < 8;
            auto go = [&]() {
                if (shape == 8) (void)hipMemcpyAsync(b, a, n16 * 16, hipMemcpyDeviceToDevice, ctx->stream);
                else if (four) hipLaunchKernelGGL(k_copy16<4>, dim3(grid), dim3(256), 0, ctx->stream, a, b, n16);
                else hipLaunchKernelGGL(k_copy16<1>, dim3(grid), dim3(256), 0, ctx->stream, a, b, n16);
            };
            go();
            SSFM_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
            for (int r = 0; r < reps; r++) go();
            SSFM_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
            SSFM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream)); SSFM_HIP_CHECK(ctx, hipGetLastError());
            float ms = 0; SSFM_HIP_CHECK(ctx, hipEventElapsedTime(&ms, e0, e1));
            best = std::max(best, 2.0 * (double)(n16 * 16) * reps / (ms * 1e-3) / 1e9);
        }
        *GBs_out = best;
        return SSFM_OK;
    };
    const int rc = body();
    if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1);
    if (a) (void)hipFree(a); if (b) (void)hipFree(b);
    return rc;
}
