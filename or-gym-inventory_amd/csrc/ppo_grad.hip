// PPO minibatch gradients of the in-library actor and critic (include/invsim.h
// "PPO gradients" states the loss; the forward half is the "MLP actor" contract,
// the backward half is defined to a tolerance).  Built with -ffp-contract=off:
// every multiply-add below is an explicit fmaf or two separately rounded
// operations, never the compiler's choice.
//
// Layout.  One workgroup walks 64-sample tiles g, g + G, ... with lane = sample
// in every wave.  Per tile:
//   gather    the tile's observation rows, through idx, cast and scaled as the
//             network's input stage does, into LDS as [input][MLP_ROW]; a sample
//             that is masked or past `rows` gets zeros, so that nothing it holds
//             can reach a sum
//   forward   mlp_forward.hpp's chunk: weights by scalar loads from the blob, one
//             fmaf per unit per input in ascending order.  Every layer keeps a
//             buffer of its own, and the last layer stores both its activation
//             (the derivative needs it) and the rescaled output
//   head      wave 0, lane = sample: d loss / d pre-activation of the output
//             units, written over the last layer's activations; the per-lane
//             stat sums stay in registers across tiles (f64)
//   backward  per layer, last to first: dW / db, one thread per (input, chunk
//             of PPO_JC units) walking the 64 samples in ascending order (x at
//             stride MLP_ROW across the lanes, delta as a broadcast); then dx
//             with lane = sample, rows of the transposed blob by scalar loads,
//             times the activation's derivative, written over the activation
// A workgroup's sums over its tiles live in its own slice of the caller's
// scratch, each word read and written by the one thread that owns it (the
// first tile stores, later ones add): no atomics, and the tile -> workgroup ->
// thread assignment is a function of `rows` and the layer shapes alone, so the
// result is deterministic.  A second launch adds the at most PPO_GROUPS
// partials of every parameter in f64 in group order, divides by the number of
// valid samples and writes torch's layouts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/invsim.h"
#include "mlp_forward.hpp"
#include "ppo_grad.hpp"

namespace invsim {
namespace {

constexpr int PPO_JC = 8;     // output units of one dW work item
constexpr int PPO_IC = 8;     // inputs of one dx chunk

// d activation / d pre-activation from the stored activation y
__device__ __forceinline__ float ppo_act_grad(float d, float y, int kind) {
    if (kind == INVSIM_MLP_RELU) return y > 0.0f ? d : 0.0f;
    if (kind == INVSIM_MLP_TANH) return d * __builtin_fmaf(-y, y, 1.0f);
    return d;
}

template <bool I64, bool CRITIC>
__global__ __launch_bounds__(512) void ppo_grad_kernel(PpoArgs a) {
    mlp_cdev m = *mlp_const(a.dev);
    using Obs = typename std::conditional<I64, long long, float>::type;
    extern __shared__ float ppo_lds[];
    const int tid = threadIdx.x, lane = tid & 63, threads = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), waves = blockDim.x >> 6;
    const int g = blockIdx.x, G = gridDim.x;
    const int nl = m.n_layers, A = m.dims[nl];
    const int64_t tiles = (a.rows + PPO_TILE - 1) / PPO_TILE;
    float *const part = a.part + (int64_t)g * a.pfloats;

    // buffer of layer l's input: rows roff(l); roff(nl) the last layer's activation, roff(nl + 1) the output
    auto roff = [&](int l) {
        int r = 0;
        for (int k = 0; k < l; k++) r += m.dims[k];
        return r;
    };
    float *const Y = ppo_lds + roff(nl) * MLP_ROW;
    float *const OUT = ppo_lds + roff(nl + 1) * MLP_ROW;

    double st[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // wave 0: this lane's stat sums over the tiles

    for (int64_t tile = g; tile < tiles; tile += G) {
        const bool first = tile == g;

        // gather
        {
            const int O = m.dims[0];
            for (int e = tid; e < PPO_TILE * O; e += threads) {
                const int smp = e / O, i = e - smp * O;
                const int64_t r = tile * PPO_TILE + smp;
                float x = 0.0f;
                if (r < a.rows) {
                    const int64_t s = a.idx ? a.idx[r] : r;
                    if (!a.valid || a.valid[s]) {
                        const Obs *row = s < a.n0 ? (const Obs *)a.obs0 + s * O : (const Obs *)a.obs + (s - a.n0) * O;
                        x = (float)row[i];
                        if (m.in_scale) x = __builtin_fmaf(x, m.in_scale[i], m.in_shift[i]);
                    }
                }
                ppo_lds[i * MLP_ROW + smp] = x;
            }
        }
        __syncthreads();

        // forward
        {
            const float *xin = ppo_lds;
            for (int l = 0; l < nl; l++) {
                const int out = m.dims[l + 1];
                const int n16 = out >> 4, n4 = ((out & 15) + 3) >> 2;
                float *xout = const_cast<float *>(xin) + m.dims[l] * MLP_ROW;
                for (int c = wave; c < n16 + n4; c += waves) {
                    if (c < n16) mlp_chunk<16, true>(m, l, 16 * c, xin, xout, OUT, lane);
                    else mlp_chunk<4, true>(m, l, 16 * n16 + 4 * (c - n16), xin, xout, OUT, lane);
                }
                __syncthreads();
                xin = xout;
            }
        }

        // head: Y <- d loss / d pre-activation of the output units (unnormalised: the reduction divides by n);
        // the actor's OUT <- d loss / d log_std per sample
        if (wave == 0) {
            const int64_t r = tile * PPO_TILE + lane;
            bool ok = r < a.rows;
            int64_t s = 0;
            if (ok) {
                s = a.idx ? a.idx[r] : r;
                ok = !a.valid || a.valid[s] != 0;
            }
            float *y = Y + lane, *o = OUT + lane;
            mlp_cfloat osc = mlp_const(m.out_scale);
            if (!ok) {
                for (int k = 0; k < A; k++) y[k * MLP_ROW] = 0.0f, o[k * MLP_ROW] = 0.0f;
            } else if constexpr (CRITIC) {
                const float err = o[0] - a.returns[s];
                st[0] += 1.0;
                st[1] += (double)err * (double)err;
                float d = 2.0f * err;
                if (osc) d = d * osc[0];
                y[0] = ppo_act_grad(d, y[0], m.out_act);
                o[0] = 0.0f;
            } else {
                mlp_cfloat sd = mlp_const(a.std), lsd = mlp_const(a.log_std);
                const float *raw = a.raw + s * A;
                float acc = a.logp0;
                for (int k = 0; k < A; k++) {
                    const float z = (raw[k] - o[k * MLP_ROW]) / sd[k];
                    acc = mlp_logp_term(acc, z, lsd[k]);
                }
                const float lr = acc - a.old_logp[s];
                const float ratio = expf(lr);
                float adv = a.adv[s];
                if (a.adv_stats) {
                    const double cnt = a.adv_stats[0];
                    if (cnt >= 2.0) adv = (float)(((double)adv - a.adv_stats[1]) / (sqrt(a.adv_stats[2] / (cnt - 1.0)) + 1e-8));
                }
                const float cl = fminf(fmaxf(ratio, a.clip_lo), a.clip_hi);
                const float s1 = adv * ratio, s2 = adv * cl;
                const bool clipped = s2 < s1;             // the clipped branch is the minimum: no gradient
                const float gl = clipped ? 0.0f : -s1;    // d loss_s / d logp
                st[0] += 1.0;
                st[1] -= (double)(clipped ? s2 : s1);
                st[3] += (double)((ratio - 1.0f) - lr);
                st[4] += (ratio < a.clip_lo || ratio > a.clip_hi) ? 1.0 : 0.0;
                st[5] += (double)ratio;
                for (int k = 0; k < A; k++) {
                    const float z = (raw[k] - o[k * MLP_ROW]) / sd[k];
                    float d = gl * (z / sd[k]);           // d logp / d mean = z / std
                    if (osc) d = d * osc[k];
                    y[k * MLP_ROW] = ppo_act_grad(d, y[k * MLP_ROW], m.out_act);
                    o[k * MLP_ROW] = gl * __builtin_fmaf(z, z, -1.0f);     // d logp / d log_std = z^2 - 1 (std tied)
                }
            }
        }
        __syncthreads();

        // backward
        for (int l = nl - 1; l >= 0; l--) {
            const int in = m.dims[l], out = m.dims[l + 1];
            float *X = ppo_lds + roff(l) * MLP_ROW;
            const float *D = X + in * MLP_ROW;
            float *P = part + a.off[l];
            // dW[j][i] and, as input `in` (x = 1), db[j]
            const int njc = (out + PPO_JC - 1) / PPO_JC, items = njc * (in + 1);
            for (int w = tid; w < items; w += threads) {
                const int jc = w / (in + 1), i = w - jc * (in + 1), j0 = jc * PPO_JC;
                const int nj = out - j0 < PPO_JC ? out - j0 : PPO_JC;
                int doff[PPO_JC];
#pragma unroll
                for (int u = 0; u < PPO_JC; u++) doff[u] = (j0 + (u < nj ? u : nj - 1)) * MLP_ROW;   // stays inside D
                float acc[PPO_JC];
#pragma unroll
                for (int u = 0; u < PPO_JC; u++) acc[u] = 0.0f;
                if (i < in) {
                    const float *x = X + i * MLP_ROW;
                    for (int s = 0; s < PPO_TILE; s++) {
                        const float xs = x[s];
#pragma unroll
                        for (int u = 0; u < PPO_JC; u++) acc[u] = __builtin_fmaf(D[doff[u] + s], xs, acc[u]);
                    }
                } else {
                    for (int s = 0; s < PPO_TILE; s++) {
#pragma unroll
                        for (int u = 0; u < PPO_JC; u++) acc[u] = acc[u] + D[doff[u] + s];
                    }
                }
#pragma unroll
                for (int u = 0; u < PPO_JC; u++) {
                    if (u < nj) {
                        float *p = i < in ? P + (int64_t)(j0 + u) * in + i : P + (int64_t)out * in + j0 + u;
                        *p = first ? acc[u] : *p + acc[u];
                    }
                }
            }
            if (!CRITIC && l == nl - 1) {       // d log_std: the head's per-sample terms, summed like a bias
                float *PL = part + a.off[nl];
                for (int k = tid; k < A; k += threads) {
                    float acc = 0.0f;
                    for (int s = 0; s < PPO_TILE; s++) acc = acc + OUT[k * MLP_ROW + s];
                    PL[k] = first ? acc : PL[k] + acc;
                }
            }
            if (l == 0) break;
            __syncthreads();
            // dx[i] = sum_j W[j][i] delta[j], times act'(x[i]), over x[i]
            const int opad = m.opad[l];
            const int nic = (in + PPO_IC - 1) / PPO_IC;
            for (int c = wave; c < nic; c += waves) {
                const int i0 = c * PPO_IC;
                const int ni = in - i0 < PPO_IC ? in - i0 : PPO_IC;
                mlp_cfloat wrow[PPO_IC];
#pragma unroll
                for (int u = 0; u < PPO_IC; u++) wrow[u] = mlp_const(m.wt[l]) + (i0 + (u < ni ? u : ni - 1)) * opad;
                float acc[PPO_IC];
#pragma unroll
                for (int u = 0; u < PPO_IC; u++) acc[u] = 0.0f;
                const float *d = D + lane;
#pragma unroll 4
                for (int j = 0; j < out; j++) {
                    const float dj = d[j * MLP_ROW];
#pragma unroll
                    for (int u = 0; u < PPO_IC; u++) acc[u] = __builtin_fmaf(wrow[u][j], dj, acc[u]);
                }
#pragma unroll
                for (int u = 0; u < PPO_IC; u++) {
                    if (u < ni) {                // wave-uniform
                        float *xp = X + (i0 + u) * MLP_ROW + lane;
                        *xp = ppo_act_grad(acc[u], *xp, m.act);
                    }
                }
            }
            __syncthreads();
        }
        __syncthreads();        // the next gather overwrites what layer 0's dW read
    }

    // this workgroup's stat partials: the lanes of wave 0, folded in a fixed order
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) {
            double v = st[k];
            for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
            if (lane == 0) a.stat_part[(int64_t)g * PPO_STATS + k] = v;
        }
    }
}

// the partials of every parameter, added in f64 in group order; / n; torch's layouts
__global__ __launch_bounds__(256) void ppo_reduce_kernel(PpoArgs a, int critic) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nl = a.n_layers;
    double n = 0.0;
    for (int g = 0; g < a.groups; g++) n += a.stat_part[(int64_t)g * PPO_STATS];
    if (p == 0 && a.stats) {
        double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int g = 0; g < a.groups; g++)
            for (int k = 1; k < 6; k++) t[k] += a.stat_part[(int64_t)g * PPO_STATS + k];
        const bool any = n > 0.0;
        a.stats[0] = n;
        a.stats[1] = any ? t[1] / n : 0.0;
        if (!critic) {
            double ent = 0.0;
            for (int k = 0; k < a.A; k++) ent += (0.5 + 0.91893853320467274178) + (double)a.log_std[k];
            a.stats[2] = any ? ent : 0.0;
            for (int k = 3; k < 6; k++) a.stats[k] = any ? t[k] / n : 0.0;
        }
    }
    const int64_t total = a.off[nl] + (critic ? 0 : a.A);
    if (p >= total) return;
    float *dst;
    bool ls = false;
    if (p >= a.off[nl]) {
        ls = true;
        dst = a.gls ? a.gls + (p - a.off[nl]) : nullptr;
    } else {
        int l = 0;
        while (l + 1 < nl && p >= a.off[l + 1]) l++;
        const int64_t q = p - a.off[l], nw = (int64_t)a.out[l] * a.in[l];
        dst = q < nw ? (a.gw[l] ? a.gw[l] + q : nullptr) : (a.gb[l] ? a.gb[l] + (q - nw) : nullptr);
    }
    if (!dst) return;
    double s = 0.0;
    for (int g = 0; g < a.groups; g++) s += (double)a.part[(int64_t)g * a.pfloats + p];
    double v = 0.0;
    if (n > 0.0) v = ls ? s / n - a.ent_coef : (s * a.scale) / n;
    *dst = (float)v;
}

}  // namespace

hipError_t ppo_prepare() {
    const void *kernels[] = {(const void *)ppo_grad_kernel<true, false>, (const void *)ppo_grad_kernel<false, false>,
                             (const void *)ppo_grad_kernel<true, true>, (const void *)ppo_grad_kernel<false, true>};
    for (const void *k : kernels) {
        hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, PPO_LDS_MAX);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t ppo_grad_launch(const MlpDev &m, const PpoArgs &a, bool i64, bool critic, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    const size_t lds = (size_t)ppo_lds_bytes(m.dims, m.n_layers);
    if (lds > (size_t)PPO_LDS_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.groups), block(mlp_threads(m));
    if (critic) {
        if (i64) hipLaunchKernelGGL((ppo_grad_kernel<true, true>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((ppo_grad_kernel<false, true>), grid, block, lds, s, a);
    } else {
        if (i64) hipLaunchKernelGGL((ppo_grad_kernel<true, false>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((ppo_grad_kernel<false, false>), grid, block, lds, s, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t total = a.off[a.n_layers] + (critic ? 0 : a.A);
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, critic ? 1 : 0);
    return hipGetLastError();
}

}  // namespace invsim
