// The part of numpy's Poisson PTRS sampler that the host and the device share:
// the constants that depend only on lam, numpy's loggam, and the host-made
// table of the acceptance test's right-hand side with its window rule.  Plain
// C++ apart from the __host__ __device__ marks, so a host-only program can
// include it without the HIP headers (tests/ptrs_table_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace invsim {

constexpr int RHS_LDS_MAX = 512;  // PTRS RHS table entries per Poisson rate (staged in LDS)

// Constants of numpy random_poisson_ptrs that depend only on lam.  For a fixed
// lam they are computed on the HOST with the reference platform's libm
// (bit-identical to what numpy computes); for per-env lam (Newsvendor) on device.
struct PtrsConst {
    double lam, slam, loglam, b, a, invalpha, vr, log_invalpha, enlam;
    double a2;        // 2 * a  (numpy evaluates 2 * a / us as (2 * a) / us)
    int32_t k0, nk;   // host table of the PTRS right-hand side for k in [k0, k0 + nk)
    int32_t toff, pad_;  // that table's offset in the handle's RHS table array
};

__host__ __device__ inline PtrsConst ptrs_const(double lam) {
    PtrsConst c;
    c.lam = lam;
    c.slam = sqrt(lam);
    c.loglam = log(lam);
    c.b = 0.931 + 2.53 * c.slam;
    c.a = -0.059 + 0.02483 * c.b;
    c.invalpha = 1.1239 + 1.1328 / (c.b - 3.4);
    c.vr = 0.9277 - 3.6224 / (c.b - 2);
    c.log_invalpha = log(c.invalpha);
    c.enlam = exp(-lam);
    c.a2 = 2 * c.a;
    c.k0 = 0;
    c.nk = 0;
    return c;
}

__host__ __device__ inline double np_loggam(double x) {
    const double a0 = 8.333333333333333e-02, a1 = -2.777777777777778e-03,
                 a2 = 7.936507936507937e-04, a3 = -5.952380952380952e-04,
                 a4 = 8.417508417508418e-04, a5 = -1.917526917526918e-03,
                 a6 = 6.410256410256410e-03, a7 = -2.955065359477124e-02,
                 a8 = 1.796443723688307e-01, a9 = -1.39243221690590e+00;
    if (x == 1.0 || x == 2.0) return 0.0;
    int64_t n = (x < 7.0) ? (int64_t)(7 - x) : 0;
    double x0 = x + (double)n;
    double x2 = (1.0 / x0) * (1.0 / x0);
    double gl0 = a9;
    gl0 *= x2; gl0 += a8;
    gl0 *= x2; gl0 += a7;
    gl0 *= x2; gl0 += a6;
    gl0 *= x2; gl0 += a5;
    gl0 *= x2; gl0 += a4;
    gl0 *= x2; gl0 += a3;
    gl0 *= x2; gl0 += a2;
    gl0 *= x2; gl0 += a1;
    gl0 *= x2; gl0 += a0;
    const double lg2pi = 1.8378770664093453e+00;
    double gl = gl0 / x0 + 0.5 * lg2pi + (x0 - 0.5) * log(x0) - x0;
    if (x < 7.0) {
        for (int64_t k = 1; k <= n; k++) {
            gl -= log(x0 - 1.0);
            x0 -= 1.0;
        }
    }
    return gl;
}

// Host table of PTRS's right-hand side  -lam + k*log(lam) - loggam(k+1)  for the
// k that occur in practice (lam +- 12 sd), evaluated with the host libm exactly as
// numpy evaluates it (distributions.c random_poisson_ptrs).  The device looks it
// up instead of computing a log-gamma per rejection test; k outside falls back.
// Appends c's entries to tab (c.toff: where they start) and sets c.k0, c.nk.
inline void rhs_table(PtrsConst &c, std::vector<double> &tab) {
    c.k0 = 0;
    c.nk = 0;
    c.toff = (int32_t)tab.size();
    if (!(c.lam >= 10) || c.lam > 1e8) return;
    const double sd = std::sqrt(c.lam);
    int64_t k0 = std::max<int64_t>(0, (int64_t)std::floor(c.lam - 12 * sd - 10));
    const int64_t k1 = (int64_t)std::ceil(c.lam + 12 * sd + 40);
    int64_t n = k1 - k0;
    if (n > RHS_LDS_MAX) {      // keep the central RHS_LDS_MAX entries (the rest: device)
        k0 = std::max<int64_t>(0, (int64_t)std::floor(c.lam) - RHS_LDS_MAX / 2 + 20);
        n = RHS_LDS_MAX;
    }
    for (int64_t k = k0; k < k0 + n; k++)
        tab.push_back(-c.lam + (double)k * c.loglam - np_loggam((double)(k + 1)));
    c.k0 = (int32_t)k0;
    c.nk = (int32_t)n;
}

}  // namespace invsim
