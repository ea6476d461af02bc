// Host check of the log-of-a-product helper behind the Cauchy cost (csrc/ssfm_math.h: LogProd, logprod_mul, logprod_flush): the flushed total against the
// extended-precision sum of the logs of the same factors, for flushes every 1, 6 and LOGPROD_MAX factors.
#include "../../spherical_sfm_amd/csrc/ssfm_math.h"
#include <cstdio>
#include <random>
#include <vector>
using namespace ssfm;
static double total(const std::vector<double>& x, int every) {
    LogProd a; double s = 0.0; int n = 0;
    for (double v : x) { if (n == every) { s += logprod_flush(a); n = 0; } logprod_mul(a, v); n++; }
    return s + logprod_flush(a);
}
static long double exact(const std::vector<double>& x) { long double s = 0; for (double v : x) s += logl((long double)v); return s; }
int main() {
    static_assert(LOGPROD_MAX == 64, "the flush rule of the kernels: at least once per 64 factors");
    std::mt19937_64 g(11); std::uniform_real_distribution<double> u(0.0, 1.0);
    int bad = 0;
    const int every[3] = {1, 6, LOGPROD_MAX};
    const double BAR = 1e-14;
    auto finite_set = [&](const char* name, const std::vector<double>& x) {
        const long double ref = exact(x);
        double t[3];
        for (int i = 0; i < 3; i++) {
            t[i] = total(x, every[i]);
            const double rel = (double)(fabsl((long double)t[i] - ref) / ref);
            std::printf("%-22s flush every %2d: total %.17g  rel. error %.3g\n", name, every[i], t[i], rel);
            if (!std::isfinite(t[i]) || !(rel <= BAR)) bad++;
        }
        for (int i = 1; i < 3; i++) if (!(fabs(t[i] - t[0]) <= BAR * fabs(t[0]))) { std::printf("%s: flush rules disagree\n", name); bad++; }
    };
    { std::vector<double> x(10000); for (double& v : x) v = 1.0 + u(g); finite_set("factors in [1, 2)", x); }
    { std::vector<double> x(2000); for (double& v : x) v = pow(10.0, 300.0 * u(g)); x[0] = 1e300; x[1] = 1e300; finite_set("factors up to 1e300", x); }
    {   // what the kernels multiply: 1 + s / b for half-pixel noise, gross outliers and residuals far below the rounding of 1 + s / b, mixed
        std::vector<double> x(4096); const double ib = 1.0 / (2.0 * 2.0);
        for (double& v : x) { const double k = u(g), r = k < 0.9 ? 0.5 * u(g) : (k < 0.95 ? 1e3 + 9e3 * u(g) : 1e-9 * u(g)); v = 1.0 + r * r * ib; }
        finite_set("Cauchy factors, mixed", x);
    }
    for (int i = 0; i < 3; i++) {
        std::vector<double> ones(1000, 1.0);
        if (total(ones, every[i]) != 0.0) { std::printf("all ones, flush every %d: %.17g, not 0\n", every[i], total(ones, every[i])); bad++; }
        std::vector<double> x(100); for (double& v : x) v = 1.0 + u(g);
        x[37] = INFINITY; if (std::isfinite(total(x, every[i]))) { std::printf("inf factor, flush every %d: finite\n", every[i]); bad++; }
        x[37] = NAN; if (std::isfinite(total(x, every[i]))) { std::printf("NaN factor, flush every %d: finite\n", every[i]); bad++; }
        x[37] = INFINITY; x[38] = NAN; if (std::isfinite(total(x, every[i]))) { std::printf("inf and NaN, flush every %d: finite\n", every[i]); bad++; }
    }
    { LogProd a; if (logprod_flush(a) != 0.0) { std::printf("empty product\n"); bad++; } }
    if (bad) { std::printf("LOGPROD_FAILED %d\n", bad); return 1; }
    std::printf("LOGPROD_OK\n");
    return 0;
}
