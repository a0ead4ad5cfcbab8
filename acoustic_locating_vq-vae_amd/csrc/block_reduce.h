// The one owner of the fixed-order reductions and scans of the device kernels (device only; included by alvq_common.h).
// The non-convolution kernels promise bitwise reproducible results: every sum runs in one order that depends on sizes alone,
// with no floating-point atomics.  The orders and the barrier contracts are written down here once:
//   wave level      wave_sum / wave_max / wave_or: xor butterfly, offsets 32, 16, ... 1; every lane ends with the result.
//                   wave_scan_incl: Hillis-Steele inclusive scan in lane order.
//   over waves      block_sum / block_max: butterfly, lane 0 of wave w stores red[k][w], one barrier, then combine_waves:
//                     kSequential  ((red[0] + red[1]) + red[2]) + ...   in wave order, starting FROM red[0], not from 0
//                     kPairwise4   (red[0] + red[1]) + (red[2] + red[3])   (4 waves only)
//                   Both orders exist in the tree and their bits differ, so the order is a named template argument; the number
//                   of waves is the extent of the LDS array.  Every thread returns with the result; a site that needs it in
//                   thread 0 only ignores it elsewhere.  block_max_or: the max of a double together with the OR of an int.
//   256-thread tree tree256_sum / tree256_max: red[t] (op)= red[t + s], s = 128, 64, ... 1.
//   scans           block_scan_excl (int, with the total), block_scan_excl_f64: wave_scan_incl, lane 63 of wave w stores
//                   sh[w], then the totals of the waves below in wave order.
//
// Starting from red[0]: 0.0 + x differs from x only for x = -0.0.  A site whose hand-written loop started from 0.0 may use
// kSequential when no wave total can be -0.0: a per-thread accumulator that starts at +0.0 and only ever adds is never -0.0
// (+0.0 + -0.0 = +0.0), and a butterfly of values that are not -0.0 cannot produce one (x + y = -0.0 needs both).  That holds at
// sum_kernel, ema_size_kernel, select_kernel (kmeans.hip) and search_kernel (tsne.hip), the four sites that used to start from
// 0.0.  A site whose per-thread value can be -0.0 (a lone product or negation, a value passed through) must say what it wants.
//
// Barrier contract (LEAD): the helpers that go through LDS write red / sh before their one internal barrier.  With LEAD = true
// they first pass a barrier of their own, so that every thread's reads of the PREVIOUS use of the same buffer are over; with
// LEAD = false the caller vouches for that: the buffer is fresh, or a barrier of the caller's already lies between, or the
// caller alternates two buffers (search_kernel: one barrier per bisection step).  After the helper returns the buffer may still
// be read by slower threads: it is free for other use only after the next barrier (tree256 with FREE = true passes it itself).
//
// Not moved, on purpose:
//   ppdist_kernel, select_kernel (kmeans.hip), room_acoustics.hip's fit sums: several values behind ONE barrier, needed in one
//                   thread each; lane 0 of each wave stores its totals itself and combine_waves supplies the order (a block_sum
//                   per candidate would cost a barrier each; fifteen sums in every thread would cost registers).
//   onehot_to_index_kernel (location.hip): three interleaved butterflies; as wave_sum / wave_or / wave_max calls the kernel
//                   takes 15 VGPRs instead of 12, in every order of the calls.
//   the arg-reductions that carry an index with their own tie rule (vq.hip's argmin kernels, relocate_kernel,
//                   room_acoustics.hip, pm_search of assign_search.h), the __shfl_down suffix scan of room_acoustics.hip, the ballot compaction of
//                   stoi_mask_kernel, and everything in conv_tile.h / wgrad_*.h.
//   the arg-max of the SRP map and the arg-min of the MUSIC null share one tie rule (the lowest index of the extremum) and one
//                   kernel, map_peak_kernel<MAXIMUM, THREADS> of steered_map.h, next to the maps it serves.
#pragma once
#include <hip/hip_runtime.h>

namespace alvq {

// ------------------------------------------------------------------------------------------------------------------ wave level
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the same, read back from lane 0 (the form the float64 kernels of kmeans.hip and tsne.hip were written with)
__device__ __forceinline__ double wave_sum_lane0(double v) { return __shfl(wave_sum(v), 0, 64); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}

// inclusive scan over the wave in lane order
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// ------------------------------------------------------------------------------------------------------------------ over waves
enum WaveOrder { kSequential, kPairwise4 };

struct OpSum {
  template <typename T> static __device__ __forceinline__ T f(T a, T b) { return a + b; }
  template <typename T> static __device__ __forceinline__ T wave(T v) { return wave_sum(v); }
};
struct OpMax {  // fmax / fmaxf: a NaN operand is dropped
  static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); }
  static __device__ __forceinline__ double f(double a, double b) { return fmax(a, b); }
  template <typename T> static __device__ __forceinline__ T wave(T v) { return wave_max(v); }
};
struct OpOr {  // the OR of an int of flags (phat_status_kernel, music_status_kernel): an OR has no order
  static __device__ __forceinline__ int f(int a, int b) { return a | b; }
  static __device__ __forceinline__ int wave(int v) { return wave_or(v); }
};
struct OpGreater {  // a > b ? a : b, the form of the spectrogram statistics' tree (a NaN in b is dropped, one in a is kept)
  template <typename T> static __device__ __forceinline__ T f(T a, T b) { return a > b ? a : b; }
};

// the WAVES wave totals red[0], red[STRIDE], ... in the named order
template <int WAVES, WaveOrder ORDER, int STRIDE = 1, typename OP = OpSum, typename T>
__device__ __forceinline__ T combine_waves(const T* red) {
  if (ORDER == kPairwise4) {
    static_assert(ORDER != kPairwise4 || WAVES == 4, "kPairwise4 combines exactly four waves");
    return OP::f(OP::f(red[0], red[STRIDE]), OP::f(red[2 * STRIDE], red[3 * STRIDE]));
  }
  T s = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) s = OP::f(s, red[w * STRIDE]);
  return s;
}

// K values a thread reduced over the workgroup of WAVES waves through red[k][wave].  LEAD: see the barrier contract.
template <WaveOrder ORDER, bool LEAD, typename OP = OpSum, typename T, int K, int WAVES>
__device__ __forceinline__ void block_sum(T (&v)[K], T (&red)[K][WAVES]) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = OP::wave(v[k]);
  if (LEAD) __syncthreads();
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < K; ++k) red[k][threadIdx.x >> 6] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = combine_waves<WAVES, ORDER, 1, OP>(red[k]);
}
// one value a thread
template <WaveOrder ORDER, bool LEAD, typename OP = OpSum, typename T, int WAVES>
__device__ __forceinline__ T block_sum(T v, T (&red)[WAVES]) {
  T a[1] = {v};
  block_sum<ORDER, LEAD, OP>(a, *(T(*)[1][WAVES])&red);
  return a[0];
}
template <WaveOrder ORDER, bool LEAD, typename T, int WAVES>
__device__ __forceinline__ T block_max(T v, T (&red)[WAVES]) { return block_sum<ORDER, LEAD, OpMax>(v, red); }

// the workgroup's maximum of v (NaN-free by construction) and the OR of flag, the waves in order; every thread gets both
template <bool LEAD, int WAVES>
__device__ __forceinline__ void block_max_or(double& v, int& flag, double (&s_max)[WAVES], int (&s_flag)[WAVES]) {
  v = wave_max(v);
  flag = wave_or(flag);
  if (LEAD) __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    s_max[threadIdx.x >> 6] = v;
    s_flag[threadIdx.x >> 6] = flag;
  }
  __syncthreads();
  v = combine_waves<WAVES, kSequential, 1, OpMax>(s_max);
  flag = s_flag[0];
#pragma unroll
  for (int i = 1; i < WAVES; ++i) flag |= s_flag[i];
}

// ------------------------------------------------------------------------------------------------------------- 256-thread tree
// red: 256 values of LDS, fresh or fenced by the caller.  Every thread returns red[0] after the tree's last barrier.  FREE:
// one more barrier, after which red may be written again (a second tree through the same buffer).
template <typename OP, bool FREE, typename T>
__device__ __forceinline__ T tree256(T v, T* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = OP::f(red[tid], red[tid + s]);
    __syncthreads();
  }
  const T r = red[0];
  if (FREE) __syncthreads();
  return r;
}
template <bool FREE, typename T>
__device__ __forceinline__ T tree256_sum(T v, T* red) { return tree256<OpSum, FREE>(v, red); }
template <bool FREE, typename T>
__device__ __forceinline__ T tree256_max(T v, T* red) { return tree256<OpGreater, FREE>(v, red); }

// ----------------------------------------------------------------------------------------------------------------------- scans
// exclusive scan over the workgroup of WAVES waves (threads in order); `total` = the sum of all
template <bool LEAD, int WAVES>
__device__ __forceinline__ int block_scan_excl(int v, int (&sh)[WAVES], int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int inc = wave_scan_incl(v);
  if (LEAD) __syncthreads();
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  constexpr int UNROLL = WAVES <= 4 ? WAVES : 4;  // 16 waves by fours: scan_kernel holds four scans; in full they cost it registers
  int before = 0;
  total = 0;
#pragma unroll UNROLL
  for (int w = 0; w < WAVES; ++w) {
    const int t = sh[w];
    if (w < wave) before += t;
    total += t;
  }
  return before + inc - v;
}

// fp64 version (leading barrier): the wave scan, then the totals of the waves below in wave order; the same on every run
__device__ __forceinline__ double block_scan_excl_f64(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double inc = wave_scan_incl(v);
  const double ex = __shfl_up(inc, 1, 64);
  __syncthreads();
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  double before = 0.0;
  for (int w = 0; w < wave; ++w) before += sh[w];
  return lane == 0 ? before : before + ex;
}

}  // namespace alvq
