// Dead-code restarts of the EMA codebook (VectorQuantizerEMA(dead_code_threshold > 0); the contract: its docstring and
// include/alvq.h).
//
// restart_gather_kernel: one workgroup (one wave) per candidate slot; the slots of one rank are s = first, first + stride, ...
// and slot s takes row rows[s / stride] of x.  A position outside [0, N) zeroes the slot and raises bit 1 of *status.
//
// restart_dead_kernel: ONE workgroup of 1024 threads does the whole restart, so the dead list never leaves LDS and no second
// launch (or workspace) is needed:
//   1. flag-and-scan over the K cluster sizes in passes of 1024 codes (code = pass * 1024 + thread, so the reads coalesce):
//      a wave ballot of "cs[k] < threshold", the lane's position from the popcount of the lower lanes, the wave totals through
//      LDS in wave order, a running total over the passes -> the dead codes in ascending order, the first R kept as uint16
//      (K <= 16384);
//   2. after a barrier (every cs has been read before any is written) the n = min(dead, R) rows are copied:
//      codebook[k] = cand[j], ema_w[k] = cand[j] * threshold (one fp32 product, no contraction), cs[k] = threshold;
//   3. counters[0] += n, counters[1] = dead.
// The launches are latency-sized (R x D = 64 x 128 floats at the speech shape); at the corner R = K = 16384, D = 512 the one
// workgroup moves 100 MB, which is accepted for what is an initialisation-sized event.
#include "alvq_common.h"

namespace alvq {

constexpr int RS_MAX_K = 16384;  // as the EMA entry points
constexpr int RS_MAX_D = 512;
constexpr int RS_THREADS = 1024;

__global__ __launch_bounds__(64) void restart_gather_kernel(const float* __restrict__ x, const int64_t* __restrict__ rows,
                                                            float* __restrict__ cand, int* status, long N, int D, int R,
                                                            int first, int stride, int vec) {
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= R || s % stride != first) return;
  const int64_t row = rows[s / stride];
  const bool ok = row >= 0 && row < N;
  if (!ok && lane == 0) atomicOr(status, 1);
  float* dst = cand + (long)s * D;
  const float* src = x + (ok ? row : 0) * D;
  if (vec) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int d = lane; d < D / 4; d += 64) ((f32x4*)dst)[d] = ok ? ((const f32x4*)src)[d] : zero;
  } else {
    for (int d = lane; d < D; d += 64) dst[d] = ok ? src[d] : 0.f;
  }
}

__global__ __launch_bounds__(RS_THREADS) void restart_dead_kernel(const float* __restrict__ cand, float* __restrict__ cs,
                                                                  float* __restrict__ W, float* __restrict__ E, const float* skip,
                                                                  int64_t* counters, int K, int D, int R, float thr, int vec) {
  __shared__ uint16_t list[RS_MAX_K];
  __shared__ int wave_tot[RS_THREADS / 64];
  if (skip && *skip != 0.f) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int dead = 0;                                   // dead codes below this pass (the same in every thread)
  for (int k0 = 0; k0 < K; k0 += RS_THREADS) {
    const int k = k0 + tid;
    const bool flag = k < K && cs[k] < thr;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) wave_tot[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RS_THREADS / 64; ++w) {
      const int t = wave_tot[w];
      if (w < wave) before += t;
      total += t;
    }
    const int pos = dead + before + __popcll(mask & ((1ull << lane) - 1ull));
    if (flag && pos < R) list[pos] = (uint16_t)k;
    dead += total;
    __syncthreads();                              // wave_tot is rewritten by the next pass; list is read below
  }
  const int n = dead < R ? dead : R;
  if (vec) {
    const int D4 = D / 4;
    for (int e = tid; e < n * D4; e += RS_THREADS) {
      const int j = e / D4, d = e - j * D4;
      const f32x4 c = ((const f32x4*)cand)[(long)j * D4 + d];
      const long o = (long)list[j] * D4 + d;
      ((f32x4*)E)[o] = c;
      ((f32x4*)W)[o] = c * thr;
    }
  } else {
    for (long e = tid; e < (long)n * D; e += RS_THREADS) {
      const int j = (int)(e / D), d = (int)(e - (long)j * D);
      const float c = cand[e];
      const long o = (long)list[j] * D + d;
      E[o] = c;
      W[o] = c * thr;
    }
  }
  for (int j = tid; j < n; j += RS_THREADS) cs[list[j]] = thr;
  if (tid == 0) {
    counters[0] += (int64_t)n;
    counters[1] = (int64_t)dead;
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace alvq

using namespace alvq;

extern "C" int alvq_vq_restart_gather_f32(const float* x, const int64_t* rows, float* cand, int* status, int64_t N, int D, int R,
                                          int first, int stride, void* stream) {
  const char* who = "alvq_vq_restart_gather_f32";
  ALVQ_REQUIRE(x && rows && cand && status, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(N > 0 && D > 0 && R > 0, ALVQ_EINVAL, "%s: bad dims N=%ld D=%d R=%d", who, (long)N, D, R);
  ALVQ_REQUIRE(D <= RS_MAX_D && R <= RS_MAX_K, ALVQ_EUNSUPPORTED, "%s: D=%d R=%d outside D <= %d, R <= %d", who, D, R, RS_MAX_D,
               RS_MAX_K);
  ALVQ_REQUIRE(stride > 0 && first >= 0 && first < stride, ALVQ_EINVAL, "%s: first=%d outside [0, stride=%d)", who, first, stride);
  const int vec = (D % 4 == 0 && aligned16(x) && aligned16(cand)) ? 1 : 0;
  hipLaunchKernelGGL(restart_gather_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, x, rows, cand, status, (long)N, D, R, first,
                     stride, vec);
  return check_launch(who);
}

extern "C" int alvq_vq_restart_dead_f32(const float* cand, float* cluster_size, float* ema_w, float* codebook, const float* skip,
                                        int64_t* counters, int K, int D, int R, float threshold, void* stream) {
  const char* who = "alvq_vq_restart_dead_f32";
  ALVQ_REQUIRE(cand && cluster_size && ema_w && codebook && counters, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(K > 0 && D > 0, ALVQ_EINVAL, "%s: bad dims K=%d D=%d", who, K, D);
  ALVQ_REQUIRE(K <= RS_MAX_K && D <= RS_MAX_D, ALVQ_EUNSUPPORTED, "%s: K=%d D=%d outside K <= %d, D <= %d", who, K, D, RS_MAX_K,
               RS_MAX_D);
  ALVQ_REQUIRE(R >= 1 && R <= K, ALVQ_EINVAL, "%s: R=%d outside [1, K=%d]", who, R, K);
  ALVQ_REQUIRE(threshold >= 0.f, ALVQ_EINVAL, "%s: threshold=%g is negative (or NaN)", who, (double)threshold);
  const int vec = (D % 4 == 0 && aligned16(cand) && aligned16(ema_w) && aligned16(codebook)) ? 1 : 0;
  hipLaunchKernelGGL(restart_dead_kernel, dim3(1), dim3(RS_THREADS), 0, (hipStream_t)stream, cand, cluster_size, ema_w, codebook,
                     skip, counters, K, D, R, threshold, vec);
  return check_launch(who);
}
