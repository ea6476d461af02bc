// spherical_sfm_amd lab -- k_band_back_lds: back substitution by one 256-thread workgroup per component behind an LDS-resident factorisation.  It was the
// fall-back for bands too wide for the single-wave k_band_back_v2; since the packed window (three task sets per lane) no band reaches it, and it left the
// library.  scripts/lab/chol_lab3.hip still times it.  LDS: band_subst_lds_bytes (csrc/band_path.h).
#pragma once
#include "band_kernels.h"

namespace ssfm {

// back substitution Y <- L^-T Y per component; next column of L prefetched into registers while the current step runs
template <int DC, int NR>
__global__ void __launch_bounds__(256)
k_band_back_lds(const double* __restrict__ band, const double* __restrict__ Linv, double* __restrict__ Y, const int* __restrict__ comp_ptr,
                int N, int b) {
    constexpr int BB = DC * DC;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* sX = lds;                               // ring [b][NR*DC]
    double* sPart = sX + (size_t)b * NR * DC;       // [b][NR*DC]
    double* sAcc = sPart + (size_t)b * NR * DC;     // NR*DC
    const int W = b + 1, n = N * DC, tid = threadIdx.x;
    const int r0 = comp_ptr[blockIdx.x], r1 = comp_ptr[blockIdx.x + 1];
    const int d = tid / DC + 1, a = tid - (d - 1) * DC;     // this lane's (offset, column) of the L column, valid if tid < b*DC
    const bool has = tid < b * DC;
    double col[DC], li[DC], yv = 0.0;
    auto fetch = [&](int j) {
#pragma unroll
        for (int m = 0; m < DC; m++) col[m] = (has && j >= r0 && j + d < r1) ? band[(((size_t)(j + d)) * W + d) * BB + m * DC + a] : 0.0;
        if (tid < NR * DC && j >= r0) {
            const int aa = tid % DC;
#pragma unroll
            for (int k = 0; k < DC; k++) li[k] = (k >= aa) ? Linv[(size_t)j * BB + k * DC + aa] : 0.0;      // column aa of L_jj^-1 = row of L^-T
            yv = Y[(size_t)(tid / DC) * n + (size_t)j * DC + aa];
        }
    };
    fetch(r1 - 1);
    int jm = (b > 0) ? (r1 - 1) % b : 0;                     // ring slot of row j, kept incrementally
    for (int j = r1 - 1; j >= r0; j--, jm = (jm == 0) ? max(b - 1, 0) : jm - 1) {
        const int nb = min(b, r1 - 1 - j);
        double cur[DC], curli[DC]; const double cury = yv;
#pragma unroll
        for (int m = 0; m < DC; m++) { cur[m] = col[m]; curli[m] = li[m]; }
        fetch(j - 1);                                   // in flight during this step
        if (has && d <= nb) {
#pragma unroll
            for (int r = 0; r < NR; r++) {
                const int xs = (jm + d >= b) ? jm + d - b : jm + d;
                const double* x = sX + ((size_t)xs * NR + r) * DC;
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < DC; m++) s += cur[m] * x[m];
                sPart[((size_t)(d - 1) * NR + r) * DC + a] = s;
            }
        }
        lds_barrier();
        if (tid < NR * DC) {
            const int r = tid / DC, aa = tid - r * DC;
            double s = cury;
            for (int dd = 0; dd < nb; dd++) s -= sPart[((size_t)dd * NR + r) * DC + aa];
            sAcc[tid] = s;
        }
        lds_barrier();
        if (tid < NR * DC) {
            const int r = tid / DC, aa = tid - r * DC;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < DC; k++) s += curli[k] * sAcc[r * DC + k];
            Y[(size_t)r * n + (size_t)j * DC + aa] = s;
            if (b > 0) sX[((size_t)jm * NR + r) * DC + aa] = s;
        }
        lds_barrier();
    }
}

}  // namespace ssfm
