// PPO minibatch gradients of the in-library actor and critic (include/invsim.h
// "PPO gradients"): the launch arguments, the scratch layout and the launcher of
// ppo_grad.hip.  No env kernel and no other network kernel sees any of this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlp_policy.hpp"

namespace invsim {

constexpr int PPO_GROUPS = 256;               // INVSIM_PPO_MAX_GROUPS
constexpr int PPO_TILE = MLP_ENVS;            // samples of one tile: lane = sample
constexpr int PPO_LDS_MAX = 160 * 1024;       // the CU's LDS: one workgroup may take all of it
constexpr int PPO_STATS = 8;                  // f64 slots of one workgroup's stat partials (6 or 2 used)

// LDS rows ([unit][MLP_ROW] floats) the gradient kernel keeps per tile: every
// layer's activations and the rescaled output beside the last layer's
inline int64_t ppo_lds_bytes(const int32_t *dims, int n_layers) {
    int64_t rows = dims[n_layers];
    for (int l = 0; l <= n_layers; l++) rows += dims[l];
    return rows * MLP_ROW * (int64_t)sizeof(float);
}

// floats of one workgroup's partial sums: per layer the weights [out][in] and
// the bias [out] (torch's layouts), then dims[n_layers] slots for log_std
inline int64_t ppo_partial_floats(const int32_t *dims, int n_layers) {
    int64_t p = dims[n_layers];
    for (int l = 0; l < n_layers; l++) p += ((int64_t)dims[l] + 1) * dims[l + 1];
    return (p + 1) / 2 * 2;
}

inline int64_t ppo_tiles(int64_t rows) { return (rows + PPO_TILE - 1) / PPO_TILE; }
inline int ppo_groups(int64_t rows) {
    const int64_t t = ppo_tiles(rows);
    return (int)(t < PPO_GROUPS ? t : PPO_GROUPS);
}

// scratch: f64 [groups][PPO_STATS] stat partials, then f32 [groups][ppo_partial_floats]
inline int64_t ppo_scratch_bytes(const int32_t *dims, int n_layers, int64_t rows) {
    return (int64_t)ppo_groups(rows) * (PPO_STATS * 8 + ppo_partial_floats(dims, n_layers) * 4);
}

// one gradient call: the gather, the head's per-sample arrays and where the
// results go.  A by-value kernel argument of the gradient kernel (the sample
// half) and of the reduction (the output half).
struct PpoArgs {
    const MlpDev *dev;                // the object's argument block in its blob
    const void *obs0, *obs;           // obs dtype; row s is s < n0 ? obs0[s] : obs[s - n0]
    int64_t n0, rows;
    const int64_t *idx;               // [rows] or null: 0 .. rows - 1
    const uint8_t *valid;             // [S] or null
    // actor
    const float *raw, *old_logp, *adv;
    const double *adv_stats;          // [3] count, mean, M2, or null
    const float *std, *log_std;       // [A], in the blob
    float logp0, clip_lo, clip_hi;    // 1 - clip_range, 1 + clip_range
    // critic
    const float *returns;
    // scratch
    double *stat_part;                // [groups][PPO_STATS]
    float *part;                      // [groups][pfloats]
    int64_t pfloats;
    int32_t groups;
    // outputs (the reduction)
    int32_t n_layers, A;
    int32_t in[MLP_LAYERS], out[MLP_LAYERS];
    int64_t off[MLP_LAYERS + 1];      // layer l's partials start at off[l]; log_std's at off[n_layers]
    float *gw[MLP_LAYERS], *gb[MLP_LAYERS];   // torch layout, entries may be null
    float *gls;                       // [A] or null
    double *stats;                    // [6] actor / [2] critic, or null
    double scale;                     // 1 (actor) or vf_coef (critic); the reduction divides by n
    double ent_coef;
};

hipError_t ppo_prepare();
// two launches: the gradient kernel over ppo_groups(rows) workgroups, then the
// reduction of their partials into the caller's tensors
hipError_t ppo_grad_launch(const MlpDev &m, const PpoArgs &a, bool i64, bool critic, hipStream_t s);

}  // namespace invsim
