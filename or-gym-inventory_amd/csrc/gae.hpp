// invsim_gae's launcher (gae.hip; include/invsim.h "Critic, GAE and parameter
// updates").  Handle-free: no env kernel and no env state is involved.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace invsim {

// one launch over [K][N] rows; term / trunc / done0 / valid may be null; returns hipGetLastError()
hipError_t gae_launch(const double *rew, const uint8_t *term, const uint8_t *trunc, const uint8_t *done0,
                      const float *value0, const float *values, int32_t K, int64_t N, double gamma, double lambda,
                      float *adv, float *ret, uint8_t *valid, hipStream_t s);

}  // namespace invsim
