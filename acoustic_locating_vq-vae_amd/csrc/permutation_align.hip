// Frequency permutation alignment of a per-bin separation (Sawada, Araki, Makino, IEEE TASLP 2011, the first, global stage):
// the classes of every bin are reordered so that class k has the same activity over time in all bins.  The definitions are the
// comment on alvq_align_permutations_f64 and alvq_permute_bins in include/alvq.h; tests/helpers/align_ref.py restates them in
// numpy.  All arithmetic is float64.  The state between iterations is perm.
//
// align_check_kernel<K>     one pass over P, a workgroup of 256 threads a bin (b, f): the K sums of the bin's rows and the count
//                       of its non-finite values behind one block_sum, then the K sums of squared deviations (the rows come from
//                       the cache the second time: 8 K T bytes a bin).  It checks perm0 and writes the bin's status, its start
//                       perm, (m, rn) of its K rows (16 bytes a row: no normalised copy of P is ever stored), score = NaN and
//                       flag = 0.  A bin of status 1 gets (m, rn) = (0, 0) and the identity, so that the centroid kernel may
//                       load through them without a branch.
// align_centroid_kernel     step 1, cac_prior_kernel's structure: the grid runs over (frame tiles of 64, b); wave k of a workgroup
//                       owns source k, a lane a frame; it walks f rising and adds u[perm[b, f, k], f, t] where the bin's status
//                       is 0 (a select, no branch), PA_STEPS bins loaded at a time.  The order over f is fixed: an item has the
//                       same bits alone or in a batch.  A batch of one at T = 500 is 8 workgroups: the f-sequential loop is the
//                       price of that order.
// align_norm_kernel         step 2, a workgroup a (b, k): sum_t c^2, then c / n in place.
// align_score_kernel<K>     step 3, a workgroup a bin: it streams the bin's K rows once against the K centroids (which lie in
//                       L2: 8 B K T bytes in all) into K^2 accumulators a thread, one block_sum brings the table together, and
//                       assign_search.h finds the winner: pm_search, assign_kernel's own search, at K <= 2 and
//                       pm_search_permutations, which walks the same candidates under the same rule six to an unranking, from
//                       K = 3.  Thread 0 writes perm, score and the bin's changed flag.
// align_changed_kernel      after the last iteration, a workgroup an item: the sum of the flags of its bins (integers).
// permute_bins_kernel<V>    out[b, k, f] = x[b, perm[b, f, k], f], a workgroup a bin, a pure copy in units V of 4, 8 or 16 bytes
//                       (the widest that divides a row), coalesced over t.
// Every sum over t is the same: thread i of 256 adds the frames t = i, i + 256, ... rising from +0.0, then
// block_sum<kSequential, true> (block_reduce.h).  No atomics, no host-side decision between the launches: status is read on
// the device.  Every grid over bins is capped at kMaxBlocks workgroups and strides over the bins beyond, whole workgroups
// at a time.  What the launches cost: DESIGN.md.
#include <cfloat>
#include <climits>
#include <cmath>

#include "array_wave.h"
#include "assign_search.h"

namespace alvq {

constexpr int PA_THREADS = 256;
constexpr int PA_WAVES = PA_THREADS / kWave;
constexpr int PA_TILE = 64;                // the frames of a workgroup of align_centroid_kernel: a lane each, in every wave
constexpr int PA_STEPS = 8;                // the bins align_centroid_kernel loads at a time
constexpr int PA_MAX_K = PM_MAX_K;
constexpr int PA_MAX_ITERATIONS = 256;

constexpr int PA_BAD_INPUT = 1;            // a non-finite value in the bin, or a perm0 row that is not a permutation

// whether p[0..K-1] is a permutation of 0..K-1; an entry out of range is never used as a shift count
__device__ __forceinline__ bool pa_is_permutation(const int* p, int K) {
  unsigned taken = 0u;
  bool ok = true;
  for (int k = 0; k < K; ++k) {
    const int j = p[k];
    if (j < 0 || j >= K || (taken & (1u << j))) ok = false;
    else taken |= 1u << j;
  }
  return ok;
}

// ------------------------------------------------------------------------------------------------ status and row statistics
template <int K>
__global__ __launch_bounds__(PA_THREADS) void align_check_kernel(const double* __restrict__ P, const int* __restrict__ perm0,
                                                                  int* __restrict__ perm, double* __restrict__ score,
                                                                  int* __restrict__ status, double2* __restrict__ rows,
                                                                  int* __restrict__ flags, long nbins, int F, int T) {
  __shared__ double s_sum[K + 1][PA_WAVES], s_dev[K][PA_WAVES];
  const int tid = threadIdx.x;
  const long row_stride = (long)F * T;
  for (long bin = blockIdx.x; bin < nbins; bin += gridDim.x) {
    const int b = (int)(bin / F), f = (int)(bin % F);
    const double* p = P + ((long)b * K * F + f) * T;

    double v[K + 1];                       // v[j]: the sum of row j; v[K]: how many values of the bin are not finite
#pragma unroll
    for (int j = 0; j <= K; ++j) v[j] = 0.0;
    for (int t = tid; t < T; t += PA_THREADS) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double x = p[j * row_stride + t];
        if (!is_finite(x)) v[K] += 1.0;
        v[j] += x;
      }
    }
    block_sum<kSequential, true>(v, s_sum);
    double m[K];
#pragma unroll
    for (int j = 0; j < K; ++j) m[j] = v[j] / (double)T;
    bool bad = v[K] != 0.0;

    double w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = 0.0;
    if (!bad)                              // the same in every thread
      for (int t = tid; t < T; t += PA_THREADS) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const double d = p[j * row_stride + t] - m[j];
          w[j] += d * d;
        }
      }
    block_sum<kSequential, true>(w, s_dev);
    if (tid != 0) continue;                // the next round's block_sum passes a barrier before it writes LDS

    int start[K];
#pragma unroll
    for (int k = 0; k < K; ++k) start[k] = perm0 ? perm0[bin * K + k] : k;
    if (perm0 && !pa_is_permutation(start, K)) bad = true;
#pragma unroll
    for (int k = 0; k < K; ++k) perm[bin * K + k] = bad ? k : start[k];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double rn = (w[j] > 0.0 && w[j] <= DBL_MAX) ? 1.0 / sqrt(w[j]) : 0.0;   // a constant row carries no evidence
      rows[((long)b * K + j) * F + f] = bad ? make_double2(0.0, 0.0) : make_double2(m[j], rn);
    }
    status[bin] = bad ? PA_BAD_INPUT : 0;
    score[bin] = NAN;                      // a bin of status 0 gets its score from align_score_kernel
    flags[bin] = 0;
  }
}

// ----------------------------------------------------------------------------------------------------------------- centroids
__global__ __launch_bounds__(kWave * PA_MAX_K) void align_centroid_kernel(const double* __restrict__ P, const int* __restrict__ perm,
                                                                           const int* __restrict__ status,
                                                                           const double2* __restrict__ rows, double* __restrict__ cent,
                                                                           int K, int F, int T) {
  const int lane = threadIdx.x & 63;
  const int k = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));          // wave k of the workgroup owns source k
  const int b = blockIdx.y, t = blockIdx.x * PA_TILE + lane;
  const bool live = t < T;
  const double* p = P + (long)b * K * F * T + (live ? t : T - 1);                  // a lane past the row reads its last frame
  const long row_stride = (long)F * T;
  double c = 0.0;
  bool seen = false;
  // A step is a chain of loads, status and perm -> (m, rn) -> P, the first three at one address for the whole wave.  Left
  // to the compiler an unrolled loop waits for every link of every step in turn; PA_STEPS steps are therefore loaded link by
  // link -- all their perm entries, then all their (m, rn), then all their frames -- and added in the order of f.
  int f = 0;
  for (; f + PA_STEPS <= F; f += PA_STEPS) {
    const long bin = (long)b * F + f;
    bool ok[PA_STEPS];
    int j[PA_STEPS];
    double2 mr[PA_STEPS];
    double x[PA_STEPS];
#pragma unroll
    for (int i = 0; i < PA_STEPS; ++i) {
      ok[i] = status[bin + i] == 0;
      j[i] = perm[(bin + i) * K + k];
    }
#pragma unroll
    for (int i = 0; i < PA_STEPS; ++i) mr[i] = rows[((long)b * K + j[i]) * F + f + i];
#pragma unroll
    for (int i = 0; i < PA_STEPS; ++i) x[i] = p[j[i] * row_stride + (long)(f + i) * T];
#pragma unroll
    for (int i = 0; i < PA_STEPS; ++i) {
      const double u = (x[i] - mr[i].x) * mr[i].y;
      const double s = seen ? c + u : u;
      c = ok[i] ? s : c;
      seen = seen || ok[i];
    }
  }
  for (; f < F; ++f) {
    const long bin = (long)b * F + f;
    const bool ok = status[bin] == 0;                  // the same in every lane; what another bin holds is loaded and dropped
    const int j = perm[bin * K + k];                   // in 0..K-1 in every bin: align_check_kernel and align_score_kernel
    const double2 mr = rows[((long)b * K + j) * F + f];
    const double u = (p[j * row_stride + (long)f * T] - mr.x) * mr.y;
    const double s = seen ? c + u : u;                 // the sum starts from the first term
    c = ok ? s : c;
    seen = seen || ok;
  }
  if (live) cent[((long)b * K + k) * T + t] = c;
}

// a workgroup a (b, k): n = sqrt(sum_t c^2); c <- c / n, or 0 where n is not > 0 and finite
__global__ __launch_bounds__(PA_THREADS) void align_norm_kernel(double* __restrict__ cent, int T) {
  __shared__ double s_red[PA_WAVES];
  const int tid = threadIdx.x;
  double* c = cent + (long)blockIdx.x * T;
  double v = 0.0;
  for (int t = tid; t < T; t += PA_THREADS) v += c[t] * c[t];
  v = block_sum<kSequential, true>(v, s_red);
  const double n = sqrt(v);
  const bool ok = n > 0.0 && n <= DBL_MAX;
  for (int t = tid; t < T; t += PA_THREADS) c[t] = ok ? c[t] / n : 0.0;
}

// -------------------------------------------------------------------------------------------------------------------- scores
template <int K>
__global__ __launch_bounds__(PA_THREADS) void align_score_kernel(const double* __restrict__ P, const double* __restrict__ cent,
                                                                  const int* __restrict__ status, const double2* __restrict__ rows,
                                                                  int* __restrict__ perm, double* __restrict__ score,
                                                                  int* __restrict__ flags, long nbins, int F, int T) {
  __shared__ double s_acc[K * K][PA_WAVES], s_table[K * K], s_score[PA_WAVES];
  __shared__ int s_rank[PA_WAVES];
  const int tid = threadIdx.x;
  const long row_stride = (long)F * T;
  int weight[PM_MAX_K];
  const int count = pm_weights(K, K, weight);
  for (long bin = blockIdx.x; bin < nbins; bin += gridDim.x) {
    // the status, the old perm, (m, rn) and the frames are all asked for before the first of them is waited for: a bin is
    // one round trip to memory, not four.  What a bin of status 1 loads (its (m, rn) are 0) is dropped below.
    const bool skip = status[bin] != 0;                // the same in the whole workgroup: nobody writes a status in this launch
    int old[K];
#pragma unroll
    for (int k = 0; k < K; ++k) old[k] = perm[bin * K + k];
    const int b = (int)(bin / F), f = (int)(bin % F);
    const double* p = P + ((long)b * K * F + f) * T;
    const double* c = cent + (long)b * K * T;
    double m[K], rn[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double2 mr = rows[((long)b * K + j) * F + f];
      m[j] = mr.x;
      rn[j] = mr.y;
    }
    double acc[K * K];                                 // acc[k K + j] = sum_t c[k, t] u[j, t]
#pragma unroll
    for (int i = 0; i < K * K; ++i) acc[i] = 0.0;
    for (int t = tid; t < T; t += PA_THREADS) {
      double u[K], ck[K];
#pragma unroll
      for (int j = 0; j < K; ++j) u[j] = p[j * row_stride + t];
#pragma unroll
      for (int k = 0; k < K; ++k) ck[k] = c[(long)k * T + t];
#pragma unroll
      for (int j = 0; j < K; ++j) u[j] = (u[j] - m[j]) * rn[j];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < K; ++j) acc[k * K + j] += ck[k] * u[j];
    }
    if (skip) continue;
    block_sum<kSequential, true>(acc, s_acc);          // its leading barrier: the previous bin's search has left s_table
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < K * K; ++i) s_table[i] = acc[i];
    }
    __syncthreads();
    PmBest best;                                       // the same winner either way (assign_search.h)
    if constexpr (K >= 3) best = pm_search_permutations<PA_THREADS, K>(s_table, true, s_score, s_rank);
    else best = pm_search<PA_THREADS>(s_table, K, K, true, weight, count, s_score, s_rank);
    if (tid != 0) continue;
    if (best.rank < 0) {                               // every permutation's score was NaN: the old perm stays
      score[bin] = NAN;
      flags[bin] = 0;
      continue;
    }
    int pi[PM_MAX_K];
    pm_unrank(best.rank, K, K, weight, pi);
    int moved = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (old[k] != pi[k]) moved = 1;
      perm[bin * K + k] = pi[k];
    }
    score[bin] = best.score;
    flags[bin] = moved;
  }
}

// a workgroup an item: changed[b] = the number of its bins whose flag is set
__global__ __launch_bounds__(PA_THREADS) void align_changed_kernel(const int* __restrict__ flags, int* __restrict__ changed, int F) {
  __shared__ int s_red[PA_WAVES];
  const int tid = threadIdx.x, b = blockIdx.x;
  int v = 0;
  for (int f = tid; f < F; f += PA_THREADS) v += flags[(long)b * F + f];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((tid & 63) == 0) s_red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) changed[b] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// -------------------------------------------------------------------------------------------------------- applying a perm
// V: the copy unit; Tv: the units of a row
template <typename V>
__global__ __launch_bounds__(PA_THREADS) void permute_bins_kernel(const V* __restrict__ x, const int* __restrict__ perm,
                                                                   V* __restrict__ out, long nbins, int K, int F, int Tv) {
  const int tid = threadIdx.x;
  const long row_stride = (long)F * Tv;
  for (long bin = blockIdx.x; bin < nbins; bin += gridDim.x) {
    const int b = (int)(bin / F), f = (int)(bin % F);
    bool ok = true;                                    // the same in every thread
    for (int k = 0; k < K; ++k) {
      const int j = perm[bin * K + k];
      if (j < 0 || j >= K) ok = false;
    }
    const long at = ((long)b * K * F + f) * Tv;
    for (int k = 0; k < K; ++k) {
      const int j = ok ? perm[bin * K + k] : k;        // a bin with an entry outside 0..K-1 passes through
      const V* src = x + at + j * row_stride;
      V* dst = out + at + k * row_stride;
      for (int t = tid; t < Tv; t += PA_THREADS) dst[t] = src[t];
    }
  }
}

}  // namespace alvq

using namespace alvq;

static bool pa_dims_ok(int B, int K, int F, int T, int min_T) {
  return B >= 1 && B <= 65535 && F >= 1 && (long)B * F <= INT_MAX && K >= 1 && K <= PA_MAX_K && T >= min_T && T <= kMaxFrames;
}

extern "C" int64_t alvq_align_workspace_bytes(int B, int K, int F, int T) {
  if (!pa_dims_ok(B, K, F, T, 2)) return -1;
  // (m, rn) of every row: (B, K, F) pairs of float64; the centroids: (B, K, T) float64; the changed flags: (B, F) int32
  return (int64_t)16 * B * K * F + (int64_t)8 * B * K * T + (int64_t)4 * B * F;
}

extern "C" int alvq_align_permutations_f64(const double* profile, const int* perm0, int* perm, double* score, int* changed,
                                           int* status, void* workspace, int B, int K, int F, int T, int iterations, void* stream) {
  const char* who = "alvq_align_permutations_f64";
  ALVQ_REQUIRE(profile && perm && score && changed && status && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_REQUIRE(K >= 1 && K <= PA_MAX_K, ALVQ_EINVAL, "%s: K=%d (need 1 <= K <= 8)", who, K);
  ALVQ_TRY(check_frames(who, T, 2));
  ALVQ_REQUIRE(iterations >= 1 && iterations <= PA_MAX_ITERATIONS, ALVQ_EINVAL, "%s: iterations=%d (need 1 <= iterations <= 256)",
               who, iterations);
  const long nbins = (long)B * F;
  hipStream_t s = (hipStream_t)stream;
  double2* rows = (double2*)workspace;
  double* cent = (double*)((char*)workspace + (int64_t)16 * B * K * F);
  int* flags = (int*)(cent + (long)B * K * T);
  const dim3 bins = capped_grid(nbins);
#define PA_CALL(N)                                                                                                           \
  hipLaunchKernelGGL((align_check_kernel<N>), bins, dim3(PA_THREADS), 0, s, profile, perm0, perm, score, status, rows, flags, \
                     nbins, F, T)
  ALVQ_FOR_1_TO_8(K, PA_CALL)
#undef PA_CALL
  const dim3 tiles((unsigned)((T + PA_TILE - 1) / PA_TILE), (unsigned)B);
  for (int it = 0; it < iterations; ++it) {
    hipLaunchKernelGGL(align_centroid_kernel, tiles, dim3(kWave * K), 0, s, profile, (const int*)perm, (const int*)status,
                       (const double2*)rows, cent, K, F, T);
    hipLaunchKernelGGL(align_norm_kernel, dim3((unsigned)(B * K)), dim3(PA_THREADS), 0, s, cent, T);
#define PA_CALL(N)                                                                                                        \
  hipLaunchKernelGGL((align_score_kernel<N>), bins, dim3(PA_THREADS), 0, s, profile, (const double*)cent, (const int*)status, \
                     (const double2*)rows, perm, score, flags, nbins, F, T)
    ALVQ_FOR_1_TO_8(K, PA_CALL)
#undef PA_CALL
  }
  hipLaunchKernelGGL(align_changed_kernel, dim3((unsigned)B), dim3(PA_THREADS), 0, s, (const int*)flags, changed, F);
  return check_launch(who);
}

template <typename V>
static void permute_bins_start(const void* x, const int* perm, void* out, long nbins, int K, int F, int Tv, hipStream_t s) {
  hipLaunchKernelGGL((permute_bins_kernel<V>), capped_grid(nbins), dim3(PA_THREADS), 0, s, (const V*)x, perm, (V*)out, nbins, K, F, Tv);
}

extern "C" int alvq_permute_bins(const void* x, const int* perm, void* out, int B, int K, int F, int T, int elem_bytes, void* stream) {
  const char* who = "alvq_permute_bins";
  ALVQ_REQUIRE(x && perm && out, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(x != out, ALVQ_EINVAL, "%s: out must not be x", who);
  ALVQ_REQUIRE(pa_dims_ok(B, K, F, T, 1), ALVQ_EINVAL,
               "%s: B=%d K=%d F=%d T=%d (need 1 <= B <= 65535, F >= 1, B F <= 2^31 - 1, 1 <= K <= 8, 1 <= T <= 65535)", who, B, K, F, T);
  ALVQ_REQUIRE(elem_bytes == 4 || elem_bytes == 8 || elem_bytes == 16, ALVQ_EINVAL, "%s: elem_bytes=%d must be 4, 8 or 16", who,
               elem_bytes);
  ALVQ_REQUIRE(((uintptr_t)x | (uintptr_t)out) % (unsigned)elem_bytes == 0, ALVQ_EINVAL, "%s: x and out must be aligned to elem_bytes",
               who);
  const long nbins = (long)B * F, row_bytes = (long)T * elem_bytes;
  const bool base16 = ((uintptr_t)x | (uintptr_t)out) % 16 == 0, base8 = ((uintptr_t)x | (uintptr_t)out) % 8 == 0;
  hipStream_t s = (hipStream_t)stream;
  // the widest unit that divides a row (every row then starts on a multiple of it)
  if (row_bytes % 16 == 0 && base16) permute_bins_start<uint4>(x, perm, out, nbins, K, F, (int)(row_bytes / 16), s);
  else if (row_bytes % 8 == 0 && base8) permute_bins_start<uint2>(x, perm, out, nbins, K, F, (int)(row_bytes / 8), s);
  else permute_bins_start<unsigned>(x, perm, out, nbins, K, F, (int)(row_bytes / 4), s);
  return check_launch(who);
}
