// The bias split reduction of the weight-gradient families whose kernels sum dY's columns themselves (bf16 / fp16, bf16x3): a
// header of its own, so that only those two translation units get a copy of the kernel (f16mx reduces its bias another way).
#pragma once
#include "alvq_common.h"

namespace alvq {

// dbias[m] (+)= scale * sum_s bias_partial[s][m], fixed order (scale: device scalar or null)
static __global__ __launch_bounds__(256) void wgrad_bias_reduce_kernel(const float* bp, float* dbias, int splits, int Mp, int M,
                                                                       int accumulate, const float* scale) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float s = 0.f;
  int k = 0;
  for (; k + 8 <= splits; k += 8) {      // eight loads in flight (one at a time is a round trip to L2 per split)
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bp[(long)(k + j) * Mp + m];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  for (; k < splits; ++k) s += bp[(long)k * Mp + m];
  if (scale) s *= *scale;
  dbias[m] = accumulate ? dbias[m] + s : s;
}

}  // namespace alvq
