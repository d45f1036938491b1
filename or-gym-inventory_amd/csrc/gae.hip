// Generalised advantage estimation over K output rows (include/invsim.h
// "Critic, GAE and parameter updates" states the recurrence op by op): a
// backward scan per env, f64, every operation rounded separately (the library
// is built with -ffp-contract=off).
//
// Layout.  Lane = env: every row access is one coalesced stream across the
// wave (8 B rewards, 4 B values, 1 B flags).  The carry is the only dependence
// between rows and no address depends on it, so the rows are walked in blocks
// of GAE_ROWS with every load of a block issued before the first operation of
// the scan: one memory latency per block instead of one per row.  The last
// block of a K that is no multiple of GAE_ROWS loads clamped (in-bounds) rows
// and skips them in the scan.  Row k needs the flags and the value of row
// k - 1 as well: they are loaded once, as row k - 1's, and handed on, so the
// kernel moves 23 B per (k, env): 14 read (reward 8, value 4, two flags), 9
// written (advantage 4, return 4, valid 1).  No LDS, no atomics: each lane
// owns its env's column.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gae.hpp"

namespace invsim {
namespace {

// Rows per block and threads per workgroup, chosen by measurement at K = 30
// on 65 536 and 1 048 576 envs (profiles/gae/table.md lists every variant).
#ifndef GAE_ROWS
#define GAE_ROWS 8
#endif
#ifndef GAE_THREADS
#define GAE_THREADS 256
#endif

__global__ void __launch_bounds__(GAE_THREADS)
gae_kernel(const double *__restrict__ rew, const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc,
           const uint8_t *__restrict__ done0, const float *__restrict__ value0, const float *__restrict__ values,
           int32_t K, int64_t N, double gamma, double gl, float *__restrict__ adv_out, float *__restrict__ ret_out,
           uint8_t *__restrict__ valid) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    constexpr int U = GAE_ROWS;
    // what row -1 stands for
    const float v0 = value0[e];
    const bool d0 = done0 ? done0[e] != 0 : false;
    // row k as the scan reaches it: its value and flags (loaded as row k's "previous row" a step earlier)
    const int64_t last = (int64_t)(K - 1) * N + e;
    float vn = values[last];
    bool te = term ? term[last] != 0 : false;
    bool dn = te | (trunc ? trunc[last] != 0 : false);
    double carry = 0.0;
    for (int k0 = K - 1; k0 >= 0; k0 -= U) {
        double r[U];
        float pv[U];
        uint8_t pte[U], ptr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {       // rows k0 - u and, for value and flags, k0 - u - 1, clamped into the arrays
            const int64_t i = (int64_t)max(k0 - u, 0) * N + e, j = (int64_t)max(k0 - u - 1, 0) * N + e;
            r[u] = rew[i];
            pv[u] = values[j];
            pte[u] = term ? term[j] : (uint8_t)0;
            ptr[u] = trunc ? trunc[j] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 - u;           // wave-uniform
            if (k < 0) break;
            const bool first = k == 0;
            const float vpf = first ? v0 : pv[u];
            const bool pte_k = !first && pte[u] != 0;
            const bool prev = first ? d0 : (pte_k | (ptr[u] != 0));
            const double vp = (double)vpf;
            const int64_t i = (int64_t)k * N + e;
            float a_f, r_f;
            if (prev) {                     // the row after a finished episode: no transition
                a_f = 0.0f;
                r_f = vpf;
                carry = 0.0;
            } else {
                const double b = te ? 0.0 : gamma * (double)vn;
                const double delta = (r[u] + b) - vp;
                const double adv = dn ? delta : delta + gl * carry;
                carry = adv;
                a_f = (float)adv;
                r_f = (float)(adv + vp);
            }
            adv_out[i] = a_f;
            ret_out[i] = r_f;
            if (valid) valid[i] = prev ? 0 : 1;
            vn = vpf, te = pte_k, dn = prev;    // row k - 1 is the next row of the scan
        }
    }
}

}  // namespace

hipError_t gae_launch(const double *rew, const uint8_t *term, const uint8_t *trunc, const uint8_t *done0,
                      const float *value0, const float *values, int32_t K, int64_t N, double gamma, double lambda,
                      float *adv, float *ret, uint8_t *valid, hipStream_t s) {
    if (K <= 0 || N <= 0) return hipSuccess;
    const int64_t blocks = (N + GAE_THREADS - 1) / GAE_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const double gl = gamma * lambda;
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)blocks), dim3(GAE_THREADS), 0, s, rew, term, trunc, done0, value0,
                       values, K, N, gamma, gl, adv, ret, valid);
    return hipGetLastError();
}

}  // namespace invsim

#ifdef GAE_STANDALONE
// Profiling only (make gae_variants, tools/gae_ab.py): this file alone as a
// shared object per (GAE_ROWS, GAE_THREADS), loaded side by side in one process.
extern "C" int gae_variant_launch(const double *rew, const uint8_t *term, const uint8_t *trunc, const uint8_t *done0,
                                  const float *value0, const float *values, int32_t K, int64_t N, double gamma,
                                  double lambda, float *adv, float *ret, uint8_t *valid, void *stream) {
    return (int)invsim::gae_launch(rew, term, trunc, done0, value0, values, K, N, gamma, lambda, adv, ret, valid,
                                   (hipStream_t)stream);
}
#endif
