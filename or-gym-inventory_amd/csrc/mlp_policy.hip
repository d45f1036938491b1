// In-library MLP actor: observations in, actions out, one launch
// (include/invsim.h "MLP actor" states the arithmetic op by op; every
// multiply-add below and in mlp_forward.hpp, which holds the forward chunk, is
// an explicit fmaf and nothing else adds or multiplies).
//
// Layout.  One workgroup = 64 envs x 4 waves (8 for wide networks:
// mlp_threads); lane = env in every wave.  The
// activations of a layer live in LDS as [unit][MLP_ROW] floats (lane reads of
// one unit: 64 consecutive words), two buffers, one workgroup barrier per
// layer.  A layer's output units are cut into chunks of 16 (then of 4 for the
// last 1..15) and dealt to the waves round-robin; mlp_forward.hpp's chunk
// keeps its accumulators in VGPRs and walks the inputs in ascending order: read x[i]
// once from LDS, one FMA per owned unit, which is the contract's order for
// every unit.  The weights of one input are contiguous over the units (the
// device copy is transposed and zero padded to a multiple of 4), indexed by
// wave-uniform values only and read through constant-address-space pointers,
// so they arrive by scalar loads and feed the FMA from SGPRs.  A padded unit is computed (its weights are 0) and dropped: it
// is never stored, so it never enters a sum.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/invsim.h"
#include "device_common.hpp"
#include "mlp_forward.hpp"
#include "mlp_policy.hpp"
#include "numpy_normal.hpp"

namespace invsim {
namespace {

// invsim.policies.convert_actions, f32 spaces
__device__ __forceinline__ float mlp_convert(float r, float lo, float hi, bool clip) {
    if (!clip) return r;
    const bool nan = r != r;
    const float x = (r > lo || nan) ? r : lo;
    return (x < hi || nan) ? x : hi;
}

// invsim.policies.convert_actions, int64 spaces: in f64
__device__ __forceinline__ long long mlp_convert(float r, double lo, double hi, bool clip) {
    double x = (double)r;
    if (clip) {
        x = x < lo ? lo : x;
        x = x > hi ? hi : x;
    }
    if (x != x) x = 0.0;
    return (long long)x;     // toward zero
}

template <class T, class... R>
__device__ __forceinline__ const T &mlp_first(const T &t, const R &...) {
    return t;
}

// SAMPLE (include/invsim.h "Gaussian MLP actor"): a compile-time variant that
// draws the action noise after the last layer.  Its MlpSample is the pack Sm,
// which is empty otherwise: the deterministic instantiations keep the
// arguments, and so the code, they had.
template <bool I64, bool SAMPLE = false, class... Sm>
__global__ __launch_bounds__(512) void mlp_policy_kernel(const MlpDev *__restrict__ mp, const void *__restrict__ obs_,
                                                         void *__restrict__ act_, float *__restrict__ raw, int64_t N,
                                                         Sm... sm_) {
    static_assert(sizeof...(Sm) == (SAMPLE ? 1 : 0), "SAMPLE takes one MlpSample");
    mlp_cdev m = *mlp_const(mp);
    using Obs = typename std::conditional<I64, long long, float>::type;
    extern __shared__ float mlp_lds[];
    const int half = m.rows * MLP_ROW;     // floats of one buffer; layer l reads buffer l & 1
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), waves = blockDim.x >> 6, threads = blockDim.x;
    const int64_t env0 = (int64_t)blockIdx.x * MLP_ENVS;

    // input: this workgroup's 64 obs rows are one contiguous block of [N][O]
    {
        const int O = m.dims[0];
        const Obs *obs = (const Obs *)obs_ + env0 * O;
        const int64_t left = (N - env0) * O;       // elements of envs < N from here on (> 0)
        for (int e = tid; e < MLP_ENVS * O; e += threads) {
            const int env = e / O, i = e - env * O;
            float x = 0.0f;                        // lanes at or past N compute on zeros and store nothing
            if (e < left) {
                x = (float)obs[e];
                if (m.in_scale) x = __builtin_fmaf(x, m.in_scale[i], m.in_shift[i]);
            }
            mlp_lds[i * MLP_ROW + env] = x;
        }
    }
    __syncthreads();

    for (int l = 0; l < m.n_layers; l++) {
        const int out = m.dims[l + 1];
        const int n16 = out >> 4, n4 = ((out & 15) + 3) >> 2;
        const float *xin = mlp_lds + (l & 1) * half;
        float *xout = mlp_lds + ((l + 1) & 1) * half;
        for (int c = wave; c < n16 + n4; c += waves) {
            if (c < n16) mlp_chunk<16, false>(m, l, 16 * c, xin, xout, nullptr, lane);
            else mlp_chunk<4, false>(m, l, 16 * n16 + 4 * (c - n16), xin, xout, nullptr, lane);
        }
        __syncthreads();
    }

    const int A = m.dims[m.n_layers];
    const float *res = mlp_lds + (m.n_layers & 1) * half;

    // sampling: wave 0, lane = env.  The env's generator draws A normals in
    // ascending action index; the sample goes to the other buffer (the last
    // layer's input, free since the barrier above, rows >= A), the epilogue
    // below spreads it.  Lanes at or past N draw nothing and store nothing.
    if constexpr (SAMPLE) {
        const MlpSample &sm = mlp_first(sm_...);
        if (wave == 0) {
            const int64_t e = env0 + lane;
            if (e < N) {
                const RngSoA rows = act_rng_rows(sm.arng, sm.npad);
                Pcg g = rows.load(e);
                float *smp = mlp_lds + ((m.n_layers + 1) & 1) * half + lane;
                mlp_cfloat sd = mlp_const(sm.std), lsd = mlp_const(sm.log_std);
                float acc = sm.logp0;
                for (int a = 0; a < A; a++) {
                    const float zf = (float)np_standard_normal(g);
                    smp[a * MLP_ROW] = __builtin_fmaf(sd[a], zf, res[a * MLP_ROW + lane]);
                    acc = mlp_logp_term(acc, zf, lsd[a]);
                }
                if (sm.logp) sm.logp[e] = acc;
                rows.store_state(e, g);
            }
        }
        __syncthreads();
    }

    // output: [N][A] rows of this workgroup's envs, contiguous again
    const int64_t left = (N - env0) * A;
    for (int e = tid; e < MLP_ENVS * A && e < left; e += threads) {
        const int env = e / A, a = e - env * A;
        float r = res[a * MLP_ROW + env];
        const int64_t g = env0 * A + e;
        if constexpr (SAMPLE) {
            const MlpSample &sm = mlp_first(sm_...);
            if (sm.mean) sm.mean[g] = r;
            r = mlp_lds[((m.n_layers + 1) & 1) * half + a * MLP_ROW + env];
        }
        if (raw) raw[g] = r;
        if (act_) {
            if (I64) ((long long *)act_)[g] = mlp_convert(r, m.clip ? m.lo_d[a] : 0.0, m.clip ? m.hi_d[a] : 0.0, m.clip != 0);
            else ((float *)act_)[g] = mlp_convert(r, m.clip ? m.lo_f[a] : 0.0f, m.clip ? m.hi_f[a] : 0.0f, m.clip != 0);
        }
    }
}

constexpr int MLP_LDS_MAX = 2 * MLP_WIDTH * MLP_ROW * (int)sizeof(float);   // 133 120 B of the CU's 160 KiB

// invsim_mlp_update: blockIdx.y = layer (n_layers: the Gaussian rows), the
// workgroups of a layer stride over its [in][opad] destination, so the stores
// are contiguous and the (small, cache-resident) source is read transposed.
// Every destination word is written: padding columns with +0.0f.
constexpr int MLP_UPD_THREADS = 256, MLP_UPD_BLOCKS = 64;
__global__ __launch_bounds__(MLP_UPD_THREADS) void mlp_update_kernel(MlpUpdate u) {
    const int l = blockIdx.y, t0 = blockIdx.x * MLP_UPD_THREADS + threadIdx.x, stride = gridDim.x * MLP_UPD_THREADS;
    if (l == u.n_layers) {
        if (u.std_src)
            for (int a = t0; a < u.A; a += stride) {
                u.std[a] = u.std_src[a];
                u.log_std[a] = u.log_std_src[a];
            }
        return;
    }
    const int in = u.in[l], out = u.out[l], opad = u.opad[l];
    if (const float *w = u.w_src[l]) {
        float *dst = u.wt[l];
        for (int d = t0; d < in * opad; d += stride) {
            const int i = d / opad, j = d - i * opad;
            dst[d] = j < out ? w[j * in + i] : 0.0f;
        }
    }
    if (const float *b = u.b_src[l]) {
        float *dst = u.bias[l];
        for (int j = t0; j < opad; j += stride) dst[j] = j < out ? b[j] : 0.0f;
    }
}

}  // namespace

hipError_t mlp_update_launch(const MlpUpdate &u, hipStream_t s) {
    hipLaunchKernelGGL(mlp_update_kernel, dim3(MLP_UPD_BLOCKS, u.n_layers + 1), dim3(MLP_UPD_THREADS), 0, s, u);
    return hipGetLastError();
}

hipError_t mlp_prepare() {
    const void *kernels[] = {(const void *)mlp_policy_kernel<true>, (const void *)mlp_policy_kernel<false>,
                             (const void *)mlp_policy_kernel<true, true, MlpSample>,
                             (const void *)mlp_policy_kernel<false, true, MlpSample>};
    for (const void *k : kernels) {
        hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, MLP_LDS_MAX);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t mlp_launch(const MlpDev &m, const MlpDev *dev, bool i64, const void *obs, void *actions, float *raw, int64_t N,
                      hipStream_t s) {
    if (N <= 0 || (!actions && !raw)) return hipSuccess;
    const size_t lds = mlp_lds_bytes(m);
    if (lds > (size_t)MLP_LDS_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((N + MLP_ENVS - 1) / MLP_ENVS)), block(mlp_threads(m));
    if (i64) hipLaunchKernelGGL(mlp_policy_kernel<true>, grid, block, lds, s, dev, obs, actions, raw, N);
    else hipLaunchKernelGGL(mlp_policy_kernel<false>, grid, block, lds, s, dev, obs, actions, raw, N);
    return hipGetLastError();
}

hipError_t mlp_sample_launch(const MlpDev &m, const MlpDev *dev, bool i64, const void *obs, void *actions, float *raw,
                             const MlpSample &sm, int64_t N, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    const size_t lds = mlp_lds_bytes(m);
    if (lds > (size_t)MLP_LDS_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((N + MLP_ENVS - 1) / MLP_ENVS)), block(mlp_threads(m));
    if (i64) hipLaunchKernelGGL((mlp_policy_kernel<true, true, MlpSample>), grid, block, lds, s, dev, obs, actions, raw, N, sm);
    else hipLaunchKernelGGL((mlp_policy_kernel<false, true, MlpSample>), grid, block, lds, s, dev, obs, actions, raw, N, sm);
    return hipGetLastError();
}

}  // namespace invsim
