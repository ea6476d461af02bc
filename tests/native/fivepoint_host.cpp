// The device functions of csrc/fivepoint_device.h compiled for the CPU (g++, no HIP): the header is plain C++ apart from its qualifiers, so with the
// qualifiers defined away and the handful of helpers it takes from the device headers supplied here, the arithmetic the kernels run can be checked
// without a GPU (tests/test_fivepoint_cpu.py) and measured (-DFP_POLISH_STEPS=0: what the elimination delivers before the polish).
// Built as a shared library; every export is one device function.
#include <algorithm>
#include <cfloat>
#include <cmath>
#define FP_HOST_HARNESS
#define __device__
#define __host__
#define __forceinline__ inline
#include "../../spherical_sfm_amd/csrc/ssfm_math.h"
using std::isfinite;
namespace ssfm {
inline double det3_dev(const double* M) { return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]); }
}
// what the workgroup-cooperative template names (it is not instantiated here)
static struct { int x; } threadIdx, blockDim;
static inline void __syncthreads() {}
static inline int atomicAdd(int* p, int v) { const int o = *p; *p += v; return o; }
#include "../../spherical_sfm_amd/csrc/fivepoint_device.h"
using namespace ssfm;

extern "C" int fp_host_solve(const double* u5, const double* v5, double* Es /* [90] row-major */) { return fp_minimal_solver(u5, v5, Es); }
extern "C" double fp_host_residual(const double* E, const double* u, const double* v) { return fp_residual(E, u, v); }
extern "C" void fp_host_decompose(const double* E, double* R1, double* R2, double* t) { fp_decompose(E, R1, R2, t); }
extern "C" int fp_host_cheirality(const double* R, const double* t, double p1x, double p1y, double p2x, double p2y) { return fp_cheirality(R, t, p1x, p1y, p2x, p2y) ? 1 : 0; }
