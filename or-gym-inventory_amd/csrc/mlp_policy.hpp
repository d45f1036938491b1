// In-library MLP actor (include/invsim.h "MLP actor"): the kernel's argument
// block and the launchers of mlp_policy.hip.  Kept apart from kernels.hpp: no
// env kernel sees any of this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace invsim {

constexpr int MLP_LAYERS = 5;     // INVSIM_MLP_MAX_LAYERS
constexpr int MLP_WIDTH = 256;    // INVSIM_MLP_MAX_WIDTH
constexpr int MLP_ENVS = 64;      // envs of one workgroup: lane = env in each of its waves
constexpr int MLP_ROW = 65;       // LDS row stride of one unit's 64 activations (floats).  65, not
                                  // 64: the input staging writes consecutive units of ONE env,
                                  // which at stride 64 all fall on one bank

// All pointers are device memory of one parameter blob (invsim_mlp), which also
// holds this block itself: the kernel takes a pointer to it.
struct MlpDev {
    int32_t n_layers, act, out_act, clip;
    int32_t dims[MLP_LAYERS + 1];     // dims[0] = obs_dim ... dims[n_layers] = action_dim
    int32_t opad[MLP_LAYERS];         // dims[l + 1] rounded up to 4: the row length of wt[l], bias[l]
    int32_t rows;                     // widest of dims[]: rows of each of the two LDS buffers
    const float *wt[MLP_LAYERS];      // [dims[l]][opad[l]]: W[l] transposed, zero padded
    const float *bias[MLP_LAYERS];    // [opad[l]] (+0.0f where the spec has no bias)
    const float *in_scale, *in_shift;     // [dims[0]] or null
    const float *out_scale, *out_shift;   // [opad[n_layers - 1]] or null
    const float *lo_f, *hi_f;             // f32 action spaces: the bounds [A]
    const double *lo_d, *hi_d;            // int64 action spaces: the bounds as f64 [A]
};

// Waves of a workgroup: 4, or 8 once a layer has 8 or more 16-unit chunks to deal
// out (a wide network's LDS leaves room for one or two workgroups per CU, and
// the second wave per SIMD hides the latency of the other's weight loads).
inline unsigned mlp_threads(const MlpDev &m) {
    int widest = 0;
    for (int l = 1; l <= m.n_layers; l++) widest = m.dims[l] > widest ? m.dims[l] : widest;
    return widest >= 128 ? 512u : 256u;
}

inline size_t mlp_lds_bytes(const MlpDev &m) { return (size_t)2 * m.rows * MLP_ROW * sizeof(float); }

// the largest dynamic LDS size the kernels may be launched with (once per device)
hipError_t mlp_prepare();
// one launch: obs [N][O] (int64 when i64, else f32) -> raw [N][A] f32 and / or
// actions [N][A] (int64 when i64, else f32); either output may be null
// `dev`: the device copy of m, which the kernel reads
hipError_t mlp_launch(const MlpDev &m, const MlpDev *dev, bool i64, const void *obs, void *actions, float *raw, int64_t N,
                      hipStream_t s);

// The sampling launch's further arguments (include/invsim.h "Gaussian MLP
// actor"): a by-value kernel argument of the sampling instantiations only.
struct MlpSample {
    float *mean;                    // [N][A]: the network's output (mlp_launch's raw), may be null
    float *logp;                    // [N], may be null
    uint64_t *arng;                 // the action generators [4][Npad] (act_rng_rows)
    int64_t npad;
    const float *std, *log_std;     // [A], in the parameter blob
    float logp0;                    // (float)(-0.5 * log(2 pi) * A)
};

// one launch: as mlp_launch with raw = the sample fmaf(std, z, mean) and actions
// = its conversion; every env < N draws A normals whatever outputs are null
hipError_t mlp_sample_launch(const MlpDev &m, const MlpDev *dev, bool i64, const void *obs, void *actions, float *raw,
                             const MlpSample &sm, int64_t N, hipStream_t s);

// invsim_mlp_update's by-value kernel argument (include/invsim.h "Critic, GAE
// and parameter updates"): per layer the caller's row-major weight / bias
// (device, null = keep) and where they go in the parameter blob.
struct MlpUpdate {
    int32_t n_layers, A;              // A: entries of std / log_std
    int32_t in[MLP_LAYERS], out[MLP_LAYERS], opad[MLP_LAYERS];
    const float *w_src[MLP_LAYERS];   // [out][in]
    const float *b_src[MLP_LAYERS];   // [out]
    float *wt[MLP_LAYERS];            // [in][opad]
    float *bias[MLP_LAYERS];          // [opad]
    const float *std_src, *log_std_src;   // [A], both or neither
    float *std, *log_std;
};

// one launch: rewrites the blob's layers (padding columns get +0.0f again) and
// the Gaussian rows; no allocation, copy or synchronisation
hipError_t mlp_update_launch(const MlpUpdate &u, hipStream_t s);

}  // namespace invsim
