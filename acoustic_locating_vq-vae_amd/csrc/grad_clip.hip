// Global-norm gradient clipping and the learning-rate schedule of the flat-buffer Adam, both as updates of its 8-float
// device state (the contract: include/alvq.h).  Neither touches an Adam kernel: all three Adam launch forms read grad_scale
// from sc[2] and lr / bias_correction1 from sc[0], so clipping is "scale sc[2] by the coefficient" and the schedule is
// "derive sc[0] from the scheduled rate".
//
// grad_sumsq_kernel: GC_PARTIALS workgroups of GC_THREADS threads, a compile-time grid -- the sum's order is a function of n
// alone, never of the device, the occupancy or the buffer's address.  The buffer is cut into quads of four floats; quad q
// belongs to thread (q mod GC_PARTIALS * GC_THREADS), which walks its quads in ascending order, four per trip (four 16-byte
// loads in flight per lane), and keeps one float64 accumulator per quad component.  The square of an fp32 value is exact in
// float64 and 2^63 x (3.4e38)^2 is far below DBL_MAX, so nothing overflows or rounds before the additions.  A buffer that is
// not 16-byte aligned, and the n mod 4 elements past the last full quad, are read with scalar loads INTO THE SAME SLOTS
// (missing components count as +0, which leaves a non-negative -- or NaN -- accumulator as it is): the result is bit for bit
// the aligned one.  Thread -> wave butterfly -> the wave sums in wave order -> partial[block].
//
// grad_clip_final_kernel: one workgroup.  The partials go through LDS and thread 0 adds them in index order -- one dependent
// chain of GC_PARTIALS float64 additions, which is what this launch costs: 512 partials of 512 threads each (the same 16 waves
// per CU as 1024 of 256) halve it, and the LDS reads of the next 16 partials are issued before the current 16 are added --
// then does the scalar arithmetic of torch.nn.utils.clip_grad_norm_ in double.  No atomics, no arrival counter: two calls on
// the same buffer give the same bits.
#include "alvq_common.h"

#include <math.h>

namespace alvq {

constexpr int GC_PARTIALS = 512;  // workgroups of the first pass (2 per CU on 256 CUs); fixed: it defines the sum's order
constexpr int GC_THREADS = 512;
constexpr int GC_BATCH = 16;      // partials thread 0 of the second pass holds in registers while the next batch is in flight
constexpr int GC_UNROLL = 4;

// components of quad q that lie in [0, n), the others as +0; vec: the buffer is 16-byte aligned and q is a full quad
__device__ __forceinline__ f32x4 load_quad(const float* __restrict__ g, long q, long nq, long n, bool vec) {
  if (vec && q < nq) return ((const f32x4*)g)[q];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const long e = q * 4;
  if (e + 0 < n) v.x = g[e + 0];
  if (e + 1 < n) v.y = g[e + 1];
  if (e + 2 < n) v.z = g[e + 2];
  if (e + 3 < n) v.w = g[e + 3];
  return v;
}

__global__ __launch_bounds__(GC_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, long n, double* __restrict__ partial,
                                                                 int vec) {
  __shared__ double wave_tot[GC_THREADS / 64];
  const long nq = n / 4, quads = (n + 3) / 4;
  const long stride = (long)GC_PARTIALS * GC_THREADS;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  long q = (long)blockIdx.x * GC_THREADS + threadIdx.x;
  // full trips: GC_UNROLL aligned quads, all below nq (no bounds test, 16-byte loads when vec)
  if (vec) {
    for (; q + (GC_UNROLL - 1) * stride < nq; q += GC_UNROLL * stride) {
      f32x4 v[GC_UNROLL];
#pragma unroll
      for (int u = 0; u < GC_UNROLL; ++u) v[u] = __builtin_nontemporal_load((const f32x4*)g + q + u * stride);
#pragma unroll
      for (int u = 0; u < GC_UNROLL; ++u) {
        const double x = (double)v[u].x, y = (double)v[u].y, z = (double)v[u].z, w = (double)v[u].w;
        a0 += x * x;
        a1 += y * y;
        a2 += z * z;
        a3 += w * w;
      }
    }
  }
  for (; q < quads; q += stride) {
    const f32x4 v = load_quad(g, q, nq, n, vec != 0);
    const double x = (double)v.x, y = (double)v.y, z = (double)v.z, w = (double)v.w;
    a0 += x * x;
    a1 += y * y;
    a2 += z * z;
    a3 += w * w;
  }
  const double t = block_sum<kSequential, false>((a0 + a1) + (a2 + a3), wave_tot);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// sc = the FlatAdam device state {lr/bc1, sqrt(bc2), grad_scale, step, skipped, norm, coef, clipped steps}
__global__ __launch_bounds__(GC_THREADS) void grad_clip_final_kernel(double* __restrict__ partial, float* __restrict__ sc,
                                                                      double max_norm, const float* __restrict__ skip) {
  __shared__ double part[GC_PARTIALS];
  for (int i = threadIdx.x; i < GC_PARTIALS; i += GC_THREADS) part[i] = partial[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double S = 0.0, next[GC_BATCH];
#pragma unroll
  for (int j = 0; j < GC_BATCH; ++j) next[j] = part[j];
  for (int i = 0; i < GC_PARTIALS; i += GC_BATCH) {
    double cur[GC_BATCH];
#pragma unroll
    for (int j = 0; j < GC_BATCH; ++j) cur[j] = next[j];
    if (i + GC_BATCH < GC_PARTIALS) {
#pragma unroll
      for (int j = 0; j < GC_BATCH; ++j) next[j] = part[i + GC_BATCH + j];
    }
#pragma unroll
    for (int j = 0; j < GC_BATCH; ++j) S += cur[j];
  }
  partial[GC_PARTIALS] = S;                              // the float64 sum of squares, for whoever wants more than sc[5]'s fp32
  const float scale = sc[2];
  const double norm = sqrt(S) * (double)scale;           // the buffer is the SUM over the ranks, sc[2] = 1/world
  sc[5] = (float)norm;
  if (skip && *skip != 0.f) {                            // the fp16-range guard's verdict: nothing of this step is applied
    sc[6] = 1.f;
    return;
  }
  double coef = max_norm / (norm + 1e-6);                // clip_grad_norm_: inf norm -> 0, NaN stays NaN (NaN > 1 is false)
  if (coef > 1.0) coef = 1.0;
  sc[6] = (float)coef;
  sc[2] = scale * (float)coef;
  if (coef < 1.0) sc[7] += 1.f;
}

// adam_advance_kernel (elementwise.hip) with sc[0] derived from the scheduled rate of the step about to be applied: linear
// warm-up lr * t / warmup for t <= warmup, then (total > warmup) cosine annealing to lr_min at t = total and lr_min after,
// else lr.  The schedule runs off the APPLIED-step counter: a step the guard skipped does not advance it.
__global__ void adam_advance_sched_kernel(float* sc, double lr, double beta1, double beta2, double grad_scale,
                                          const float* prev_skip, int* range_flag, int* range_sticky, double warmup, double total,
                                          double lr_min) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double t = (double)sc[3];
  if (prev_skip && *prev_skip != 0.f) sc[4] += 1.f;
  else t += 1.0;
  if (prev_skip && range_flag) {
    const int f = *range_flag;
    if (f) { *range_sticky |= f; *range_flag = 0; }
  }
  const double tt = t < 1.0 ? 1.0 : t;        // as adam_advance_kernel: a skipped very first step is retried as step 1
  double lr_t = lr;
  if (tt <= warmup) {
    lr_t = lr * tt / warmup;
  } else if (total > warmup) {
    double p = (tt - warmup) / (total - warmup);
    if (p > 1.0) p = 1.0;
    lr_t = lr_min + (lr - lr_min) * (0.5 * (1.0 + cos(M_PI * p)));
  }
  sc[0] = (float)(lr_t / (1.0 - pow(beta1, tt)));
  sc[1] = (float)sqrt(1.0 - pow(beta2, tt));
  sc[2] = (float)grad_scale;
  sc[3] = (float)t;
}

}  // namespace alvq

using namespace alvq;

extern "C" int64_t alvq_grad_clip_workspace_bytes(int64_t n) {
  ALVQ_REQUIRE(n > 0, -1, "alvq_grad_clip_workspace_bytes: n <= 0");
  return (int64_t)(GC_PARTIALS + 1) * (int64_t)sizeof(double);
}

extern "C" int alvq_grad_clip_f32(const float* grad, int64_t n, float* scalars, double max_norm, void* workspace,
                                  const float* skip, void* stream) {
  const char* who = "alvq_grad_clip_f32";
  ALVQ_REQUIRE(grad && scalars && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(n > 0, ALVQ_EINVAL, "%s: n <= 0", who);
  ALVQ_REQUIRE(max_norm > 0.0, ALVQ_EINVAL, "%s: max_norm=%g is not positive (or is NaN)", who, max_norm);
  ALVQ_REQUIRE(((uintptr_t)grad & 3) == 0 && ((uintptr_t)workspace & 7) == 0, ALVQ_EINVAL, "%s: misaligned pointer", who);
  hipStream_t s = (hipStream_t)stream;
  const int vec = ((uintptr_t)grad & 15) == 0 ? 1 : 0;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(GC_PARTIALS), dim3(GC_THREADS), 0, s, grad, (long)n, (double*)workspace, vec);
  hipLaunchKernelGGL(grad_clip_final_kernel, dim3(1), dim3(GC_THREADS), 0, s, (double*)workspace, scalars, max_norm, skip);
  return check_launch(who);
}

extern "C" int alvq_adam_advance_sched_f32(float* scalars, double lr, double beta1, double beta2, double grad_scale,
                                           const float* prev_skip, void* stream, int64_t warmup_steps, int64_t total_steps,
                                           double lr_min) {
  const char* who = "alvq_adam_advance_sched_f32";
  ALVQ_REQUIRE(scalars, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(warmup_steps >= 0 && total_steps >= 0, ALVQ_EINVAL, "%s: negative step count", who);
  ALVQ_REQUIRE(total_steps == 0 || total_steps > warmup_steps, ALVQ_EINVAL, "%s: total_steps=%ld is not beyond warmup_steps=%ld",
               who, (long)total_steps, (long)warmup_steps);
  ALVQ_REQUIRE(lr_min >= 0.0, ALVQ_EINVAL, "%s: lr_min=%g is negative (or NaN)", who, lr_min);
  int* flag = prev_skip ? fx_range_flag_ptr() : nullptr;
  int* sticky = prev_skip ? fx_range_sticky_ptr() : nullptr;
  ALVQ_REQUIRE(!prev_skip || (flag && sticky), ALVQ_EINVAL, "%s: the range flag's device address is unavailable", who);
  hipLaunchKernelGGL(adam_advance_sched_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scalars, lr, beta1, beta2, grad_scale,
                     prev_skip, flag, sticky, (double)warmup_steps, (double)total_steps, lr_min);
  return check_launch(who);
}
