// Launchers of the running-normalisation calls (norm.hip; include/invsim.h
// "Running normalisation").  Handle-free but for mlp_set_rows_launch, which
// writes into an invsim_mlp's blob: no env kernel and no env state is involved.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace invsim {

// bytes of scratch invsim_moments needs for any dtype: every level of partial nodes below the root
int64_t moments_scratch_bytes(int64_t rows, int32_t cols);

// leaves + tree + Merge(stats, batch); dtype is INVSIM_DTYPE_*; mask may be null; returns hipGetLastError()
hipError_t moments_launch(const void *x, int32_t dtype, int64_t rows, int32_t cols, const uint8_t *mask, double *stats,
                          double *scratch, hipStream_t s);

// forward scan per env over [K][N] rows; term / trunc / done0 / valid may be null
hipError_t discounted_returns_launch(const double *rew, const uint8_t *term, const uint8_t *trunc, const uint8_t *done0,
                                     int32_t K, int64_t N, double gamma, double *ret, double *out, uint8_t *valid,
                                     hipStream_t s);

// out[i] = clamp(reward[i] / sqrt(var + epsilon)); stats is [3][1]
hipError_t normalize_rewards_launch(const double *rew, int64_t count, const double *stats, double epsilon, double clip,
                                    double *out, hipStream_t s);

// scale[c] = (float)(1 / sqrt(var + epsilon)), shift[c] = (float)(-(mean * inv)); shift may be null
hipError_t norm_params_launch(const double *stats, int32_t cols, double epsilon, float *scale, float *shift, hipStream_t s);

// two [n] f32 rows, device to device
hipError_t mlp_set_rows_launch(float *dst_scale, float *dst_shift, const float *scale, const float *shift, int32_t n,
                               hipStream_t s);

}  // namespace invsim
