// The one definition of the forward arithmetic of include/invsim.h's "MLP
// actor" contract.  The actor kernels (mlp_policy.hip) and the forward half of
// the gradient kernels (ppo_grad.hip) instantiate it, so a change to the chunk
// reaches both and the learner's log-probabilities stay bitwise the rollout's.
// Every multiply-add is an explicit fmaf and nothing else adds or multiplies.
#pragma once
#include "../../include/invsim.h"
#include "mlp_policy.hpp"

namespace invsim {
namespace {

// The parameter blob is written before a launch (at create, or by an earlier
// mlp_update_kernel launch, whose stores are visible at this one's start) and
// only read by the network kernels: pointers into it are taken in the constant
// address space, so every wave-uniform read of it (the argument block, weights,
// biases, output scales) is a scalar load whatever the compiler can prove about
// aliasing.
#define MLP_CONST __attribute__((address_space(4)))
typedef const float MLP_CONST *mlp_cfloat;
typedef const MlpDev MLP_CONST &mlp_cdev;
template <typename T>
__device__ __forceinline__ const T MLP_CONST *mlp_const(const T *p) {
    return (const T MLP_CONST *)(uintptr_t)p;
}

__device__ __forceinline__ float mlp_activate(float v, int kind) {
    if (kind == INVSIM_MLP_RELU) return v > 0.0f ? v : 0.0f;   // NaN -> +0.0f
    if (kind == INVSIM_MLP_TANH) return tanhf(v);
    return v;
}

// one action's term of the Gaussian log-probability: acc - z^2 / 2 - log_std
__device__ __forceinline__ float mlp_logp_term(float acc, float z, float log_std) {
    acc = __builtin_fmaf(-0.5f * z, z, acc);
    return acc - log_std;
}

// CH output units base .. base + CH - 1 of layer l for this wave's 64 envs.
// KEEP = false, the actor: xout gets the activated and, on the last layer,
// rescaled value; yout is unused.  KEEP = true, the gradient kernels: xout gets
// the activation (the derivative needs it), the last layer's yout the rescaled.
template <int CH, bool KEEP>
__device__ __forceinline__ void mlp_chunk(mlp_cdev m, int l, int base, const float *xin, float *xout, float *yout,
                                          int lane) {
    const int in = m.dims[l], out = m.dims[l + 1], opad = m.opad[l];
    const bool last = l == m.n_layers - 1;
    mlp_cfloat w = mlp_const(m.wt[l]) + base;
    mlp_cfloat b = mlp_const(m.bias[l]) + base;
    mlp_cfloat osc = mlp_const(m.out_scale), osh = mlp_const(m.out_shift);
    float acc[CH];
#pragma unroll
    for (int u = 0; u < CH; u++) acc[u] = b[u];
    const float *x = xin + lane;
#pragma unroll 4
    for (int i = 0; i < in; i++, w += opad, x += MLP_ROW) {
        const float xi = *x;
#pragma unroll
        for (int u = 0; u < CH; u++) acc[u] = __builtin_fmaf(w[u], xi, acc[u]);
    }
    const int kind = last ? m.out_act : m.act;
    const bool scale = last && m.out_scale;
#pragma unroll
    for (int u = 0; u < CH; u++) {
        if (base + u < out) {        // wave-uniform
            if constexpr (KEEP) {
                const float v = mlp_activate(acc[u], kind);
                xout[(base + u) * MLP_ROW + lane] = v;
                if (last) yout[(base + u) * MLP_ROW + lane] = scale ? __builtin_fmaf(v, osc[base + u], osh[base + u]) : v;
            } else {
                float v = mlp_activate(acc[u], kind);
                if (scale) v = __builtin_fmaf(v, osc[base + u], osh[base + u]);
                xout[(base + u) * MLP_ROW + lane] = v;
            }
        }
    }
}

}  // namespace
}  // namespace invsim
