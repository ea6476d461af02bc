// spherical_sfm_amd -- the share of a Gram task that one wave of its workgroup takes (ba_kernels.h: schur_gram_task<..., SPLIT = true>).
//
// A task is a run of cnt points walked in sub-chunks of GRAM_SHARE_SUB points; with W waves per task, wave w takes a contiguous run of WHOLE sub-chunks
// [s_begin, s_end) (in points; only the task's last sub-chunk may be partial).  The nsub = ceil(cnt / 8) sub-chunks are dealt evenly: nsub / W each, the
// first nsub % W waves one more -- the longest share is ceil(nsub / W), and a share is empty only when there are fewer sub-chunks than waves (the rule of
// k_gram_backsub2, ceil(nsub / W) for every wave until none are left, has the same longest share but leaves a wave idle at e.g. 5 sub-chunks on 4 waves).
// Host-compilable: tests/native/gram_split_check.cpp.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SSFM_SHARE_HD __host__ __device__ __forceinline__
#else
#define SSFM_SHARE_HD inline
#endif

namespace ssfm {
constexpr int GRAM_SHARE_SUB = 8;       // points per sub-chunk (= GRAM_SUB_PTS of ba_flatten.h)
SSFM_SHARE_HD void gram_share(int cnt, int W, int w, int& s_begin, int& s_end) {
    const int nsub = (cnt + GRAM_SHARE_SUB - 1) / GRAM_SHARE_SUB, base = nsub / W, rem = nsub - base * W;
    const int b = w * base + (w < rem ? w : rem), n = base + (w < rem ? 1 : 0);
    s_begin = b * GRAM_SHARE_SUB < cnt ? b * GRAM_SHARE_SUB : cnt;
    s_end = (b + n) * GRAM_SHARE_SUB < cnt ? (b + n) * GRAM_SHARE_SUB : cnt;
}
}  // namespace ssfm
