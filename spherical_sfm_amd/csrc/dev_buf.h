// spherical_sfm_amd -- device buffers of the entry points: DevBuf (pooled allocation, ssfm_ctx.h: DevPool), the scope that frees an entry point's temporaries,
// and the two ways a host array reaches the device (upload, StagedUploads).  Everything a unit needs that launches no BA or band kernel.
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <tuple>
#include <vector>
#include "ssfm_ctx.h"

namespace ssfm {

static double wall_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// SSFM_PLAN_TIMING: time spent in hipMalloc (atomic: the observation arrays are allocated by the upload thread of ba_create_impl while the main thread plans)
static bool g_alloc_timing = false; static std::atomic<long long> g_alloc_ns{0}; static std::atomic<int> g_alloc_n{0};
template <typename T>
struct DevBuf {
    T* p = nullptr; size_t n = 0; size_t cap_bytes = 0; int dev = 0;
    hipError_t alloc(size_t count) {
        n = count;
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        const double t0 = g_alloc_timing ? wall_s() : 0.0;
        (void)hipGetDevice(&dev);
        hipError_t e = hipSuccess;
        p = static_cast<T*>(g_dev_pool.take(bytes, dev, &cap_bytes));
        if (!p) {
            e = hipMalloc((void**)&p, bytes); cap_bytes = bytes;
            if (e != hipSuccess) {                    // the pool may be sitting on the memory: give it back to the driver and try once more
                (void)hipGetLastError(); g_dev_pool.drain(dev);
                e = hipMalloc((void**)&p, bytes);
                if (e != hipSuccess) { p = nullptr; cap_bytes = 0; }
            }
        }
        if (g_alloc_timing) { g_alloc_ns += (long long)(1e9 * (wall_s() - t0)); g_alloc_n++; }
        return e;
    }
    void free() {
        if (p && cap_bytes > 0 && g_dev_pool.give(p, cap_bytes, dev)) { p = nullptr; n = 0; cap_bytes = 0; return; }   // recycled (ssfm_ctx.h: DevPool)
        if (p) (void)hipFree(p);
        p = nullptr; n = 0; cap_bytes = 0;
    }
};
// Frees the buffers it was given, in the order given, when it leaves scope: the temporaries of an entry point, whichever way the entry point
// returns.  DevBuf itself has no destructor (a handle's buffers are freed by free_all after its stream is synchronised).  The scope does not
// synchronise: on the path without an error the entry point has done so before the scope ends (ssfm_ctx.h: DevPool's RULE).  On an early return after
// a failed HIP call the buffers go to the pool unsynchronised, as the probes have always done; ransac.hip's solver_probe, which used to leak them
// there instead, now does the same.
template <typename... B>
struct DevBufScope {
    std::tuple<B&...> bufs;
    explicit DevBufScope(B&... b) : bufs(b...) {}
    DevBufScope(const DevBufScope&) = delete;
    ~DevBufScope() { std::apply([](auto&... b) { (b.free(), ...); }, bufs); }
};

template <typename T, typename A>
static hipError_t upload(DevBuf<T>& b, const std::vector<T, A>& v, hipStream_t s) {
    hipError_t e = b.alloc(v.size()); if (e != hipSuccess) return e;
    if (v.empty()) return hipSuccess;
    return hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
}

// Small host arrays through the context's pinned staging buffer (round 6): a pageable hipMemcpyAsync stages and waits inside the call -- the ~25 arrays of a pose-graph
// solve's set-up were 25 copies of 2-5 us with the host's 4-20 us between them (rocprofv3 trace: 210 us); from pinned memory the calls return at once and the copies
// run back to back.  reserve() before the first up(): the buffer is grow-only and must not move while copies are in flight; an array that does not fit takes upload().
struct StagedUploads {
    ssfm_ctx* ctx; hipStream_t st; size_t off = 0;
    StagedUploads(ssfm_ctx* c, hipStream_t s) : ctx(c), st(s) {}
    hipError_t reserve(size_t bytes) {
        const size_t want = (bytes + 7) / 8 + 64;
        if (ctx->dl_stage_n >= want) return hipSuccess;
        if (ctx->dl_stage) (void)hipHostFree(ctx->dl_stage);
        ctx->dl_stage = nullptr; ctx->dl_stage_n = 0;
        const size_t n = want + want / 2;
        hipError_t e = hipHostMalloc((void**)&ctx->dl_stage, n * sizeof(double), hipHostMallocDefault);
        if (e == hipSuccess) ctx->dl_stage_n = n; else { ctx->dl_stage = nullptr; (void)hipGetLastError(); }
        return hipSuccess;                                             // (no pinned memory: every up() falls back to upload())
    }
    template <typename T, typename A>
    hipError_t up(DevBuf<T>& b, const std::vector<T, A>& v) {
        const size_t bytes = v.size() * sizeof(T), need = (bytes + 63) / 64 * 64;
        if (!ctx->dl_stage || off + need > ctx->dl_stage_n * sizeof(double)) return upload(b, v, st);
        hipError_t e = b.alloc(v.size()); if (e != hipSuccess) return e;
        if (v.empty()) return hipSuccess;
        char* dst = reinterpret_cast<char*>(ctx->dl_stage) + off; off += need;
        std::memcpy(dst, v.data(), bytes);
        return hipMemcpyAsync(b.p, dst, bytes, hipMemcpyHostToDevice, st);
    }
};

}  // namespace ssfm
