// How good a separation is, measured on the device in float64: the SI-SDR of every (reference, estimate) pair of an item, the
// best assignment of estimates to references, and the scale-invariant SDR / SIR / SAR split (Le Roux et al. 2019).  The
// definitions are the comments on alvq_pairwise_si_sdr_*, alvq_assign_f64 and alvq_si_bss_eval_* in include/alvq.h;
// tests/helpers/separation_metrics_ref.py restates them in numpy.
//
// No atomics and nothing compared across workgroups: every sum runs in one order that depends on the row's own sizes alone, so
// an item has the same bits in any batch and on any run.  No workspace, no host sync, one launch each.
//   pairwise_si_sdr_kernel  a workgroup per (item, reference): si_sdr_kernel (speech_metrics.hip) with J estimates at once.  The
//                           reference row is read once per pass for all J estimates; 1 + J, 1 + J and 2 J running sums a
//                           thread.  Each sum is si_sdr_kernel's own (the samples t = thread, thread + 256, ..., then
//                           block_sum<kSequential, true>, three passes), so an entry has the bits si_sdr_kernel gives the pair.
//   assign_kernel           a workgroup per item: pm_search (assign_search.h, shared with permutation_align.hip) -- the threads
//                           stride over the ranks of the injections, unrank each through the factorial number system and keep
//                           their best (score, rank); an arg-reduction over (score, rank) with the same rule (ties to the
//                           lowest rank) picks the winner -- which thread 0 unranks once more.
//   si_bss_eval_kernel      a workgroup per (item, reference i): pass 1, the means of the K references and of the chosen
//                           estimate, and a count of the non-finite samples of the K estimates the item's perm row selects (so
//                           that every workgroup of an item arrives at the same status); pass 2, the upper triangle of the Gram
//                           matrix and g, K (K + 1) / 2 + K sums a thread; thread 0 solves G c = g in LDS; pass 3, the five
//                           energies.  The K workgroups of an item each build G: the price of one launch without scratch.
#include <cfloat>
#include <cmath>

#include "array_wave.h"
#include "assign_search.h"

namespace alvq {

constexpr int PM_THREADS = 256;
constexpr int PM_WAVES = PM_THREADS / kWave;
constexpr int PM_MAX_N = 1 << 24;
constexpr int PM_MAX_ITEMS = 65535;        // items ride on gridDim.y

constexpr int PM_BAD_INPUT = 1;            // a reference of zero or non-finite centred energy, or a non-finite estimate sample
constexpr int PM_BAD_SOLVE = 2;            // a pivot that is 0 or not finite
constexpr int PM_BAD_PERM = 3;             // a perm row that is not an injection into 0..J-1
constexpr int PM_NONE_VALID = 1;           // assign: every injection's score was NaN

// 10 log10(num / den) under the rules of si_sdr_kernel: NaN for a NaN energy, +inf for a denominator of 0
__device__ __forceinline__ double pm_ratio_db(double num, double den) {
  if (num != num || den != den) return NAN;
  if (den == 0.0) return INFINITY;
  return 10.0 * log10(num / den);
}

// ------------------------------------------------------------------------------------------------------------ pairwise SI-SDR
template <typename T, int J>
__global__ __launch_bounds__(PM_THREADS) void pairwise_si_sdr_kernel(const T* __restrict__ references,
                                                                     const T* __restrict__ estimates, double* __restrict__ table,
                                                                     int K, int n) {
  __shared__ double s_dot[1 + J][PM_WAVES], s_energy[2 * J][PM_WAVES];
  const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
  const T* s = references + ((long)b * K + i) * n;
  const T* e = estimates + (long)b * J * n;
  double* out = table + ((long)b * K + i) * J;

  double v[1 + J];                         // v[0]: the reference's; v[1 + j]: estimate j's
#pragma unroll
  for (int j = 0; j <= J; ++j) v[j] = 0.0;
  for (int t = tid; t < n; t += PM_THREADS) {
    v[0] += (double)s[t];
#pragma unroll
    for (int j = 0; j < J; ++j) v[1 + j] += (double)e[(long)j * n + t];
  }
  block_sum<kSequential, true>(v, s_dot);
  const double ms = v[0] / (double)n;
  double me[J];
#pragma unroll
  for (int j = 0; j < J; ++j) me[j] = v[1 + j] / (double)n;

#pragma unroll
  for (int j = 0; j <= J; ++j) v[j] = 0.0;
  for (int t = tid; t < n; t += PM_THREADS) {
    const double a = (double)s[t] - ms;
    v[0] += a * a;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const double c = (double)e[(long)j * n + t] - me[j];
      v[1 + j] += c * a;
    }
  }
  block_sum<kSequential, true>(v, s_dot);
  const double ss = v[0];
  if (!(ss > 0.0 && ss <= DBL_MAX)) {
    if (tid < J) out[tid] = NAN;
    return;
  }
  double alpha[J], w[2 * J];               // w[2 j]: |target|^2, w[2 j + 1]: |target - e_j|^2
#pragma unroll
  for (int j = 0; j < J; ++j) {
    alpha[j] = v[1 + j] / ss;
    w[2 * j] = w[2 * j + 1] = 0.0;
  }
  for (int t = tid; t < n; t += PM_THREADS) {
    const double a = (double)s[t] - ms;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const double target = alpha[j] * a, c = (double)e[(long)j * n + t] - me[j];
      w[2 * j] += target * target;
      w[2 * j + 1] += (target - c) * (target - c);
    }
  }
  block_sum<kSequential, true>(w, s_energy);
  if (tid != 0) return;
#pragma unroll
  for (int j = 0; j < J; ++j) out[j] = pm_ratio_db(w[2 * j], w[2 * j + 1]);
}

// ---------------------------------------------------------------------------------------------------------------- assignment
__global__ __launch_bounds__(PM_THREADS) void assign_kernel(const double* __restrict__ table, int* __restrict__ perm,
                                                            double* __restrict__ total, int* __restrict__ status, int K, int J,
                                                            int maximize) {
  __shared__ double s_table[PM_MAX_K * PM_MAX_K], s_score[PM_WAVES];
  __shared__ int s_rank[PM_WAVES];
  const int tid = threadIdx.x, b = blockIdx.x;
  const bool up = maximize != 0;
  if (tid < K * J) s_table[tid] = table[(long)b * K * J + tid];
  __syncthreads();
  int weight[PM_MAX_K];
  const int count = pm_weights(K, J, weight);
  const PmBest best = pm_search<PM_THREADS>(s_table, K, J, up, weight, count, s_score, s_rank);   // assign_search.h
  if (tid != 0) return;
  int pi[PM_MAX_K];
  if (best.rank < 0) {
    for (int k = 0; k < K; ++k) perm[(long)b * K + k] = k;
    total[b] = NAN;
    status[b] = PM_NONE_VALID;
    return;
  }
  pm_unrank(best.rank, K, J, weight, pi);
  for (int k = 0; k < K; ++k) perm[(long)b * K + k] = pi[k];
  total[b] = best.score;
  status[b] = 0;
}

// ----------------------------------------------------------------------------------------------------------- SI-SDR, SIR, SAR
// G c = g in LDS by one thread: the rule of iva_solve (iva_kernels.h) for a real matrix.  m: K rows of K + 1, the last column
// the right-hand side, which the solution replaces.  False where a pivot is 0 or not finite.
__device__ bool pm_solve(double (*m)[PM_MAX_K + 1], int K) {
  for (int j = 0; j < K; ++j) {
    int p = j;
    double top = fabs(m[j][j]);
    for (int r = j + 1; r < K; ++r)
      if (fabs(m[r][j]) > top) {
        p = r;
        top = fabs(m[r][j]);
      }
    if (!(top > 0.0 && top <= DBL_MAX)) return false;
    if (p != j)
      for (int c = 0; c <= K; ++c) {
        const double x = m[j][c];
        m[j][c] = m[p][c];
        m[p][c] = x;
      }
    for (int r = j + 1; r < K; ++r) {
      const double l = m[r][j] / m[j][j];
      for (int c = j; c <= K; ++c) m[r][c] -= l * m[j][c];
    }
  }
  for (int j = K - 1; j >= 0; --j) {
    m[j][K] = m[j][K] / m[j][j];
    for (int r = 0; r < j; ++r) m[r][K] -= m[r][j] * m[j][K];
  }
  return true;
}

template <typename T, int K>
__global__ __launch_bounds__(PM_THREADS) void si_bss_eval_kernel(const T* __restrict__ references, const T* __restrict__ estimates,
                                                                 const int* __restrict__ perm, double* __restrict__ sdr,
                                                                 double* __restrict__ sir, double* __restrict__ sar,
                                                                 int* __restrict__ status, int J, int n) {
  constexpr int PAIRS = K * (K + 1) / 2;
  __shared__ double s_mean[K + 2][PM_WAVES], s_gram[PAIRS + K][PM_WAVES], s_energy[5][PM_WAVES];
  __shared__ double s_m[PM_MAX_K][PM_MAX_K + 1];
  __shared__ int s_ok;
  const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
  const long row = (long)b * K + i;

  // the item's perm row: every entry in 0..J-1 and no column twice, before any estimate is read
  int pi[K];
  unsigned taken = 0u;
  bool injective = true;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    pi[k] = perm[(long)b * K + k];
    if (pi[k] < 0 || pi[k] >= J || (taken & (1u << pi[k]))) injective = false;
    else taken |= 1u << pi[k];
  }
  if (!injective) {
    if (tid == 0) {
      sdr[row] = sir[row] = sar[row] = NAN;
      if (i == 0) status[b] = PM_BAD_PERM;
    }
    return;
  }
  const T* s = references + (long)b * K * n;
  const T* est = estimates + (long)b * J * n;
  const T* e = est + (long)pi[i] * n;

  // pass 1: the sums of the K references and of the chosen estimate; how many samples of the selected estimates are not finite
  double v[K + 2];
#pragma unroll
  for (int k = 0; k < K + 2; ++k) v[k] = 0.0;
  for (int t = tid; t < n; t += PM_THREADS) {
#pragma unroll
    for (int p = 0; p < K; ++p) {
      v[p] += (double)s[(long)p * n + t];
      const double x = (double)est[(long)pi[p] * n + t];
      if (!is_finite(x)) v[K + 1] += 1.0;
      if (p == i) v[K] += x;
    }
  }
  block_sum<kSequential, true>(v, s_mean);
  double ms[K];
#pragma unroll
  for (int p = 0; p < K; ++p) ms[p] = v[p] / (double)n;
  const double me = v[K] / (double)n;
  const bool bad_sample = v[K + 1] != 0.0;

  // pass 2: G[p][q], p <= q, row after row, then g[p]
  double u[PAIRS + K];
#pragma unroll
  for (int k = 0; k < PAIRS + K; ++k) u[k] = 0.0;
  for (int t = tid; t < n; t += PM_THREADS) {
    double a[K];
#pragma unroll
    for (int p = 0; p < K; ++p) a[p] = (double)s[(long)p * n + t] - ms[p];
    const double c = (double)e[t] - me;
    int at = 0;
#pragma unroll
    for (int p = 0; p < K; ++p)
#pragma unroll
      for (int q = p; q < K; ++q) u[at++] += a[p] * a[q];
#pragma unroll
    for (int p = 0; p < K; ++p) u[PAIRS + p] += c * a[p];
  }
  block_sum<kSequential, true>(u, s_gram);

  bool bad_energy = false;
  double gii = 0.0;
  {
    int at = 0;
#pragma unroll
    for (int p = 0; p < K; ++p) {
      if (!(u[at] > 0.0 && u[at] <= DBL_MAX)) bad_energy = true;
      if (p == i) gii = u[at];
      at += K - p;
    }
  }
  double gi = 0.0;
#pragma unroll
  for (int p = 0; p < K; ++p)
    if (p == i) gi = u[PAIRS + p];
  const bool own_energy = gii > 0.0 && gii <= DBL_MAX;
  int code = (bad_energy || bad_sample) ? PM_BAD_INPUT : 0;

  // c = G^-1 g by thread 0
  if (tid == 0) {
    int at = 0;
#pragma unroll
    for (int p = 0; p < K; ++p)
#pragma unroll
      for (int q = p; q < K; ++q) {
        s_m[p][q] = s_m[q][p] = u[at];
        ++at;
      }
#pragma unroll
    for (int p = 0; p < K; ++p) s_m[p][K] = u[PAIRS + p];
    s_ok = code == 0 ? (pm_solve(s_m, K) ? 1 : 0) : 1;
  }
  __syncthreads();
  if (code == 0 && !s_ok) code = PM_BAD_SOLVE;
  if (tid == 0 && i == 0) status[b] = code;
  if (!own_energy) {                       // si_sdr_kernel's NaN; the item has status 1
    if (tid == 0) sdr[row] = sir[row] = sar[row] = NAN;
    return;
  }
  double coef[K];
#pragma unroll
  for (int p = 0; p < K; ++p) coef[p] = code == 0 ? s_m[p][K] : 0.0;
  const double alpha = gi / gii;

  // pass 3: |target|^2, |target - e|^2, |interf|^2, |artif|^2, |proj|^2
  double w[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = tid; t < n; t += PM_THREADS) {
    double a[K];
#pragma unroll
    for (int p = 0; p < K; ++p) a[p] = (double)s[(long)p * n + t] - ms[p];
    const double c = (double)e[t] - me;
    double ai = a[0];
#pragma unroll
    for (int p = 1; p < K; ++p)
      if (p == i) ai = a[p];
    const double target = alpha * ai;
    double proj = coef[0] * a[0];
#pragma unroll
    for (int p = 1; p < K; ++p) proj += coef[p] * a[p];
    const double interf = proj - target, artif = c - proj;
    w[0] += target * target;
    w[1] += (target - c) * (target - c);
    w[2] += interf * interf;
    w[3] += artif * artif;
    w[4] += proj * proj;
  }
  block_sum<kSequential, true>(w, s_energy);
  if (tid != 0) return;
  sdr[row] = pm_ratio_db(w[0], w[1]);
  sir[row] = code == 0 ? pm_ratio_db(w[0], w[2]) : NAN;
  sar[row] = code == 0 ? pm_ratio_db(w[4], w[3]) : NAN;
}

}  // namespace alvq

using namespace alvq;

static int pm_check_dims(const char* who, int B, int K, int J, int n) {
  ALVQ_REQUIRE(B >= 1 && B <= PM_MAX_ITEMS && K >= 1 && K <= PM_MAX_K && J >= 1 && J <= PM_MAX_K && n >= 2 && n <= PM_MAX_N,
               ALVQ_EINVAL, "%s: B=%d K=%d J=%d n=%d (need 1 <= B <= 65535, 1 <= K, J <= 8, 2 <= n <= 2^24)", who, B, K, J, n);
  return ALVQ_OK;
}

template <typename T>
static int pairwise_si_sdr_launch(const char* who, const T* references, const T* estimates, double* table, int B, int K, int J,
                                  int n, void* stream) {
  ALVQ_REQUIRE(references && estimates && table, ALVQ_EINVAL, "%s: null pointer", who);
  const int rc = pm_check_dims(who, B, K, J, n);
  if (rc != ALVQ_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
#define PM_CALL(N) \
  hipLaunchKernelGGL((pairwise_si_sdr_kernel<T, N>), dim3(K, B), dim3(PM_THREADS), 0, s, references, estimates, table, K, n)
  ALVQ_FOR_1_TO_8(J, PM_CALL)
#undef PM_CALL
  return check_launch(who);
}

extern "C" int alvq_pairwise_si_sdr_f32(const float* references, const float* estimates, double* table, int B, int K, int J, int n,
                                        void* stream) {
  return pairwise_si_sdr_launch("alvq_pairwise_si_sdr_f32", references, estimates, table, B, K, J, n, stream);
}

extern "C" int alvq_pairwise_si_sdr_f64(const double* references, const double* estimates, double* table, int B, int K, int J, int n,
                                        void* stream) {
  return pairwise_si_sdr_launch("alvq_pairwise_si_sdr_f64", references, estimates, table, B, K, J, n, stream);
}

extern "C" int alvq_assign_f64(const double* table, int* perm, double* total, int* status, int B, int K, int J, int maximize,
                               void* stream) {
  const char* who = "alvq_assign_f64";
  ALVQ_REQUIRE(table && perm && total && status, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(B >= 1 && B <= PM_MAX_ITEMS && K >= 1 && K <= J && J <= PM_MAX_K, ALVQ_EINVAL,
               "%s: B=%d K=%d J=%d (need 1 <= B <= 65535, 1 <= K <= J <= 8)", who, B, K, J);
  ALVQ_REQUIRE(maximize == 0 || maximize == 1, ALVQ_EINVAL, "%s: maximize=%d must be 0 or 1", who, maximize);
  hipLaunchKernelGGL(assign_kernel, dim3(B), dim3(PM_THREADS), 0, (hipStream_t)stream, table, perm, total, status, K, J, maximize);
  return check_launch(who);
}

template <typename T>
static int si_bss_eval_launch(const char* who, const T* references, const T* estimates, const int* perm, double* sdr, double* sir,
                              double* sar, int* status, int B, int K, int J, int n, void* stream) {
  ALVQ_REQUIRE(references && estimates && perm && sdr && sir && sar && status, ALVQ_EINVAL, "%s: null pointer", who);
  const int rc = pm_check_dims(who, B, K, J, n);
  if (rc != ALVQ_OK) return rc;
  ALVQ_REQUIRE(K <= J, ALVQ_EINVAL, "%s: K=%d J=%d (need K <= J: every reference takes an estimate of its own)", who, K, J);
  hipStream_t s = (hipStream_t)stream;
#define PM_CALL(N)                                                                                                          \
  hipLaunchKernelGGL((si_bss_eval_kernel<T, N>), dim3(N, B), dim3(PM_THREADS), 0, s, references, estimates, perm, sdr, sir, sar, \
                     status, J, n)
  ALVQ_FOR_1_TO_8(K, PM_CALL)
#undef PM_CALL
  return check_launch(who);
}

extern "C" int alvq_si_bss_eval_f32(const float* references, const float* estimates, const int* perm, double* sdr, double* sir,
                                    double* sar, int* status, int B, int K, int J, int n, void* stream) {
  return si_bss_eval_launch("alvq_si_bss_eval_f32", references, estimates, perm, sdr, sir, sar, status, B, K, J, n, stream);
}

extern "C" int alvq_si_bss_eval_f64(const double* references, const double* estimates, const int* perm, double* sdr, double* sir,
                                    double* sar, int* status, int B, int K, int J, int n, void* stream) {
  return si_bss_eval_launch("alvq_si_bss_eval_f64", references, estimates, perm, sdr, sir, sar, status, B, K, J, n, stream);
}
