// The one owner of the exhaustive assignment search that alvq_assign_f64 defines (include/alvq.h), device only: assign_kernel
// (separation_metrics.hip) and align_score_kernel (permutation_align.hip) both call it, so the two cannot drift apart.
// The injections pi of {0..K-1} into {0..J-1} are ranked in lexicographic order; the score of pi is
// table[0][pi(0)] + table[1][pi(1)] + ..., k rising from the first term; a NaN score is skipped; the winner has the largest
// (smallest) score and the lowest rank among equal scores.  The threads stride over the ranks, unrank each through the
// factorial number system and keep their best (score, rank); an arg-reduction over (score, rank) with the same rule (ties to
// the lowest rank) picks the winner, so the result does not depend on which thread saw which rank.
#pragma once
#include <hip/hip_runtime.h>

namespace alvq {

constexpr int PM_MAX_K = 8;

struct PmBest {
  double score;
  int rank;                                // -1: nothing yet
};

// whether candidate (s, r) beats `best` under the rule: a valid one beats none; the larger (smaller) score; then the lower rank
__device__ __forceinline__ bool pm_beats(double s, int r, const PmBest& best, bool maximize) {
  if (r < 0) return false;
  if (best.rank < 0) return true;
  if (s != best.score) return maximize ? s > best.score : s < best.score;
  return r < best.rank;
}

// the injection of rank `rank` in lexicographic order: position k takes the digit-th smallest column not yet taken, the digits
// those of rank in the mixed radix (J, J - 1, ..., J - K + 1); weight[k] = (J - k - 1)(J - k - 2) ... (J - K + 1)
__device__ __forceinline__ void pm_unrank(int rank, int K, int J, const int* weight, int* pi) {
  unsigned taken = 0u;
  for (int k = 0; k < K; ++k) {
    int digit = rank / weight[k];
    rank -= digit * weight[k];
    int col = 0;
    for (;; ++col) {                       // digit < J - k columns are free: col stays below J
      if (taken & (1u << col)) continue;
      if (digit == 0) break;
      --digit;
    }
    taken |= 1u << col;
    pi[k] = col;
  }
}

// weight[] of pm_unrank; returns the number of injections, J (J - 1) ... (J - K + 1)
__device__ __forceinline__ int pm_weights(int K, int J, int* weight) {
  int count = 1;
  for (int k = K - 1; k >= 0; --k) {
    weight[k] = count;
    count *= J - k;
  }
  return count;
}

// The arg-reduction over the threads' best (score, rank) by a workgroup of THREADS threads: the xor butterfly over the wave,
// then thread 0 over the waves, under pm_beats.  The winner is valid in thread 0 only; s_score / s_rank: THREADS / 64 entries
// of LDS.  One barrier inside; the caller fences s_score and s_rank before it reuses them.
template <int THREADS>
__device__ __forceinline__ PmBest pm_reduce(PmBest best, bool up, double* s_score, int* s_rank) {
  const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double s = __shfl_xor(best.score, o, 64);
    const int r = __shfl_xor(best.rank, o, 64);
    if (pm_beats(s, r, best, up)) best = PmBest{s, r};
  }
  if (lane == 0) {
    s_score[tid >> 6] = best.score;
    s_rank[tid >> 6] = best.rank;
  }
  __syncthreads();
  if (tid != 0) return best;
  for (int w = 1; w < THREADS / 64; ++w)
    if (pm_beats(s_score[w], s_rank[w], best, up)) best = PmBest{s_score[w], s_rank[w]};
  return best;
}

// The search over s_table (K rows of J, in LDS, written and fenced by the caller) by a workgroup of THREADS threads.  The
// winner is valid in thread 0 only (rank -1: every injection was skipped).  pm_reduce's barrier inside; the caller fences
// s_table, s_score and s_rank before it reuses them.
template <int THREADS>
__device__ __forceinline__ PmBest pm_search(const double* s_table, int K, int J, bool up, const int* weight, int count,
                                            double* s_score, int* s_rank) {
  PmBest best = {0.0, -1};
  int pi[PM_MAX_K];
  for (int rank = threadIdx.x; rank < count; rank += THREADS) {
    pm_unrank(rank, K, J, weight, pi);
    double s = s_table[pi[0]];
    for (int k = 1; k < K; ++k) s += s_table[k * J + pi[k]];
    if (s != s) continue;
    if (pm_beats(s, rank, best, up)) best = PmBest{s, rank};   // the ranks of a thread rise: an equal score never replaces
  }
  return pm_reduce<THREADS>(best, up, s_score, s_rank);
}

// The same search, with the same winner, for the K! permutations of a K x K table whose K >= 3 is known at compile time.  A
// permutation's rank is 6 times the rank of its first K - 3 entries among the injections of K - 3 positions into K columns,
// plus the rank of its last three entries among the six orders of the three columns left; so a thread strides over the
// K! / 6 prefixes, unranks each once, keeps its partial score, and walks the six suffixes in lexicographic order from nine
// table entries in registers: a sixth of the unrankings and a third of the LDS reads of pm_search.  A score is still
// table[0][pi(0)] + table[1][pi(1)] + ..., k rising from the first term, so it has pm_search's bits, and (score, rank) under
// pm_beats is a total order: the winner does not depend on how the candidates were walked.
template <int THREADS, int K>
__device__ __forceinline__ PmBest pm_search_permutations(const double* s_table, bool up, double* s_score, int* s_rank) {
  static_assert(K >= 3 && K <= PM_MAX_K, "three columns are left to the suffix");
  constexpr int P = K - 3;
  int weight[PM_MAX_K], pi[PM_MAX_K];
  const int count = pm_weights(P, K, weight);          // K (K - 1) ... 4 = K! / 6; 1 for K = 3
  PmBest best = {0.0, -1};
  for (int prefix = threadIdx.x; prefix < count; prefix += THREADS) {
    pm_unrank(prefix, P, K, weight, pi);
    unsigned left = (1u << K) - 1u;
    double part = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      left &= ~(1u << pi[k]);
      part = k == 0 ? s_table[pi[0]] : part + s_table[k * K + pi[k]];
    }
    int r[3];                                          // the three columns left, rising
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      r[i] = __ffs(left) - 1;
      left &= left - 1u;
    }
    double a[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) a[i][j] = s_table[(P + i) * K + r[j]];
    constexpr int order[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = P == 0 ? a[0][order[i][0]] : part + a[0][order[i][0]];
      s += a[1][order[i][1]];
      s += a[2][order[i][2]];
      if (s != s) continue;
      if (pm_beats(s, 6 * prefix + i, best, up)) best = PmBest{s, 6 * prefix + i};   // a thread's ranks rise here too
    }
  }
  return pm_reduce<THREADS>(best, up, s_score, s_rank);
}

}  // namespace alvq
