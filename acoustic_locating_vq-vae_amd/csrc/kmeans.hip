// k-means (sklearn.cluster.KMeans(algorithm="lloyd") semantics; the contract in full: the docstring of
// acoustic_locating_vq_vae/kmeans.py) around the quantiser's argmin, which is the assignment step (alvq_vq_argmin_f32).
//
// Kernels, every sum in one fixed order (no floating-point atomics), so results are bitwise reproducible:
//   hist_kernel        one wave per block of KM_SB rows: per-block label counts and each row's stable rank among the rows of
//                      its label in the block (64-row chunks in order, ranks within a chunk by lane); "labels changed" flag.
//   scan_kernel        one workgroup: exclusive scan of the counts in (cluster, block) order -> each row's sorted position;
//                      cluster starts / counts, the centre-sum segments (KM_SEG rows each) and the number of empty clusters.
//   scatter_kernel     perm[position] = row: the rows sorted by label, stably (row order within a label).
//   segsum_kernel      one workgroup per segment: fp64 column sums of its rows in row order.
//   clustersum_kernel  one workgroup per cluster: its segments' sums in segment order.
//   rowdist_kernel     one wave per row: |x - c[label]|^2 in fp64 (relocation: old centres; inertia: final centres).
//   relocate_kernel    one workgroup, only when a cluster is empty: sklearn's _relocate_empty_clusters_dense.
//   finalize_kernel    one workgroup per cluster: centre = fl32(sum * (1 / count)), the shift |c_new - c_old|.
//   verdict_kernel     one workgroup: center_shift_tot = sum shift^2 and the convergence verdict.
// The EMA quantiser (VectorQuantizerEMA) takes its per-code statistics from the first five (hist .. clustersum, fp32 out) and
// updates its state with ema_size_kernel (one workgroup: cluster sizes, their fp64 total, Laplace smoothing) and
// ema_apply_kernel (elementwise: moving-average sums, codebook = sums / sizes).
// k-means++ (greedy, sklearn's _kmeans_plusplus): per round, pick_kernel (one workgroup: the candidates by a blocked fp64
// inclusive cumsum of closest_dist_sq), ppdist_kernel (64 rows per workgroup: candidate-to-row distances, min with the
// closest, per-block potentials) and select_kernel (one workgroup: the candidate of least potential).  Three launches a round,
// no host read: K rounds are one capturable launch chain.
#include <cmath>

#include "alvq_common.h"

namespace alvq {

constexpr int KM_SB = 1024;     // rows per label block (hist / scatter)
constexpr int KM_SEG = 128;     // rows per centre-sum segment
constexpr int KM_MAX_K = 16384; // label counts of a block live in LDS (64 KB)
constexpr int KM_MAX_D = 512;   // as the argmin
constexpr int KM_CS_ROWS = 512; // rows per column-statistics chunk
constexpr int PP_ROWS = 64;     // rows per k-means++ block
constexpr int PP_DC = 128;      // dims per staged chunk
constexpr int PP_MAX_T = 16;    // candidates per round (one wave each in pick_kernel)

// ---------------------------------------------------------------------------------------------------- Lloyd update
__global__ __launch_bounds__(64) void hist_kernel(const int64_t* __restrict__ labels, const int64_t* __restrict__ labels_old,
                                                  int* __restrict__ H, int* __restrict__ rank, int* __restrict__ blk_changed,
                                                  long N, int K, int NB) {
  extern __shared__ int cnt[];  // [K]
  const int lane = threadIdx.x, b = blockIdx.x;
  for (int k = lane; k < K; k += 64) cnt[k] = 0;
  __syncthreads();
  bool changed = false;
  const long r0 = (long)b * KM_SB;
  for (int c = 0; c < KM_SB / 64; ++c) {
    const long r = r0 + c * 64 + lane;
    int L = -1;
    if (r < N) {
      const int64_t l = labels[r];
      if (!labels_old || labels_old[r] != l) changed = true;
      L = (l >= 0 && l < K) ? (int)l : -1;
    }
    int below = 0;
    bool last = true;
    for (int j = 0; j < 64; ++j) {
      const int o = __shfl(L, j, 64);
      if (o == L) {
        if (j < lane) ++below;
        else if (j > lane) last = false;
      }
    }
    const int base = L >= 0 ? cnt[L] : 0;
    if (L >= 0) rank[r] = base + below;
    __syncthreads();
    if (L >= 0 && last) cnt[L] = base + below + 1;
    __syncthreads();
  }
  const bool any = __ballot(changed) != 0;
  for (int k = lane; k < K; k += 64) H[(long)k * NB + b] = cnt[k];
  if (lane == 0) blk_changed[b] = any ? 1 : 0;
}

// state[0] labels changed, [1] empty clusters, [2] segments
__global__ __launch_bounds__(1024) void scan_kernel(int* __restrict__ HO, const int* __restrict__ blk_changed, int* __restrict__ start,
                                                    int* __restrict__ cnt, int* __restrict__ seg_start, int* __restrict__ state,
                                                    int K, int NB) {
  __shared__ int sh[16];
  const int tid = threadIdx.x;
  const long M = (long)K * NB, per = (M + 1023) / 1024;
  const long lo = min(M, tid * per), hi = min(M, lo + per);
  int s = 0;
  for (long e = lo; e < hi; ++e) s += HO[e];
  int total = 0;
  int ex = block_scan_excl<true>(s, sh, total);
  for (long e = lo; e < hi; ++e) {
    const int v = HO[e];
    HO[e] = ex;
    ex += v;
  }
  __threadfence_block();
  __syncthreads();
  const int perk = (K + 1023) / 1024;
  const int klo = min(K, tid * perk), khi = min(K, klo + perk);
  int segs = 0, empty = 0;
  for (int k = klo; k < khi; ++k) {
    const int st = HO[(long)k * NB], en = k + 1 < K ? HO[(long)(k + 1) * NB] : total;
    start[k] = st;
    cnt[k] = en - st;
    segs += (en - st + KM_SEG - 1) / KM_SEG;
    empty += en == st;
  }
  int nseg = 0;
  int sx = block_scan_excl<true>(segs, sh, nseg);
  for (int k = klo; k < khi; ++k) {
    seg_start[k] = sx;
    sx += (cnt[k] + KM_SEG - 1) / KM_SEG;
  }
  int n_empty = 0;
  (void)block_scan_excl<true>(empty, sh, n_empty);
  int ch = 0;
  for (int b = tid; b < NB; b += 1024) ch |= blk_changed[b];
  int n_changed = 0;
  (void)block_scan_excl<true>(ch, sh, n_changed);
  if (tid == 0) {
    seg_start[K] = nseg;
    state[0] = n_changed > 0;
    state[1] = n_empty;
    state[2] = nseg;
  }
}

__global__ __launch_bounds__(256) void scatter_kernel(const int64_t* __restrict__ labels, const int* __restrict__ HO,
                                                      const int* __restrict__ rank, int* __restrict__ perm, long N, int K, int NB) {
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < N; r += (long)gridDim.x * 256) {
    const int64_t l = labels[r];
    if (l < 0 || l >= K) continue;
    perm[HO[l * NB + r / KM_SB] + rank[r]] = (int)r;
  }
}

__global__ __launch_bounds__(128) void segsum_kernel(const float* __restrict__ x, const int* __restrict__ perm,
                                                     const int* __restrict__ start, const int* __restrict__ cnt,
                                                     const int* __restrict__ seg_start, const int* __restrict__ state,
                                                     double* __restrict__ part, int K, int D) {
  __shared__ int rows[KM_SEG];
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= state[2]) return;
  int lo = 0, hi = K;  // seg_start[lo] <= g < seg_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_start[mid] <= g) lo = mid;
    else hi = mid;
  }
  const int j = g - seg_start[lo];
  const int r0 = start[lo] + j * KM_SEG, n = min(KM_SEG, cnt[lo] - j * KM_SEG);
  if (tid < n) rows[tid] = perm[r0 + tid];
  __syncthreads();
  double acc[KM_MAX_D / 128] = {};
  for (int i = 0; i < n; ++i) {
    const float* xr = x + (long)rows[i] * D;
#pragma unroll
    for (int q = 0; q < KM_MAX_D / 128; ++q) {
      const int d = tid + 128 * q;
      if (d < D) acc[q] += (double)xr[d];
    }
  }
#pragma unroll
  for (int q = 0; q < KM_MAX_D / 128; ++q) {
    const int d = tid + 128 * q;
    if (d < D) part[(long)g * D + d] = acc[q];
  }
}

// TS, TC: double / int for the Lloyd update; float / float for the EMA quantiser's statistics (the fp64 sum rounded once)
template <typename TS, typename TC>
__global__ __launch_bounds__(128) void clustersum_kernel(const double* __restrict__ part, const int* __restrict__ seg_start,
                                                         const int* __restrict__ cnt, TS* __restrict__ sums,
                                                         TC* __restrict__ wcnt, int D) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const int g0 = seg_start[k], g1 = seg_start[k + 1];
  for (int d = tid; d < D; d += 128) {
    double s = 0.0;
    for (int g = g0; g < g1; ++g) s += part[(long)g * D + d];
    sums[(long)k * D + d] = (TS)s;
  }
  if (tid == 0) wcnt[k] = (TC)cnt[k];
}

// dist[r] = |x_r - c[label_r]|^2 in fp64; skipped entirely when gate != NULL and *gate == 0
__global__ __launch_bounds__(256) void rowdist_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels,
                                                      const float* __restrict__ c, double* __restrict__ dist, const int* gate,
                                                      long N, int K, int D) {
  if (gate && *gate == 0) return;
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < N; r += (long)gridDim.x * 4) {
    const int64_t l = labels[r];
    double s = 0.0;
    if (l >= 0 && l < K)
      for (int d = lane; d < D; d += 64) {
        const double v = (double)x[r * D + d] - (double)c[l * D + d];
        s += v * v;
      }
    s = wave_sum_lane0(s);
    if (lane == 0) dist[r] = s;
  }
}

// sklearn's _relocate_empty_clusters_dense with a defined order: rows by distance (to the OLD centre of their label)
// descending, ties to the lower row index, paired with the empty clusters in ascending order.  Nothing moves when the
// largest distance is 0.  The far row's values replace the empty cluster's sum (count 1) and leave its old cluster's.
__global__ __launch_bounds__(1024) void relocate_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels,
                                                        const double* __restrict__ dist, double* __restrict__ sums,
                                                        int* __restrict__ wcnt, int* __restrict__ elist, int* __restrict__ state,
                                                        long N, int K, int D) {
  __shared__ int sh[16];
  __shared__ double bd_s[16];
  __shared__ long br_s[16];
  __shared__ long far_s;
  __shared__ double far_d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ne = state[1];
  if (ne == 0) {
    if (tid == 0) state[3] = 0;
    return;
  }
  const int perk = (K + 1023) / 1024;
  const int klo = min(K, tid * perk), khi = min(K, klo + perk);
  int mine = 0;
  for (int k = klo; k < khi; ++k) mine += wcnt[k] == 0;
  int total = 0;
  int pos = block_scan_excl<true>(mine, sh, total);
  for (int k = klo; k < khi; ++k)
    if (wcnt[k] == 0) elist[pos++] = k;
  __threadfence_block();
  __syncthreads();
  double pd = __builtin_inf();
  long pr = -1;
  int moved = 0;
  for (int j = 0; j < ne; ++j) {
    // the largest (d, -r) strictly after (pd, -pr) in the order
    double bd = -1.0;
    long br = N;
    for (long r = tid; r < N; r += 1024) {
      const double d = dist[r];
      const bool after = d < pd || (d == pd && r > pr);
      if (after && (d > bd || (d == bd && r < br))) {
        bd = d;
        br = r;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double od = __shfl_xor(bd, o, 64);
      const long orr = __shfl_xor(br, o, 64);
      if (od > bd || (od == bd && orr < br)) {
        bd = od;
        br = orr;
      }
    }
    if (lane == 0) {
      bd_s[wave] = bd;
      br_s[wave] = br;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 16; ++w)
        if (bd_s[w] > bd || (bd_s[w] == bd && br_s[w] < br)) {
          bd = bd_s[w];
          br = br_s[w];
        }
      far_s = br;
      far_d = bd;
    }
    __syncthreads();
    const long f = far_s;
    const double fd = far_d;
    if (j == 0 && !(fd > 0.0)) break;  // the largest distance is 0: relocating is pointless (sklearn)
    if (f >= N || fd < 0.0) break;
    const int e = elist[j], o = (int)labels[f];
    for (int d = tid; d < D; d += 1024) {
      const double v = (double)x[f * D + d];
      sums[(long)o * D + d] -= v;
      sums[(long)e * D + d] = v;
    }
    if (tid == 0) {
      wcnt[e] = 1;
      wcnt[o] -= 1;
    }
    ++moved;
    pd = fd;
    pr = f;
    __syncthreads();
  }
  if (tid == 0) state[3] = moved;
}

__global__ __launch_bounds__(128) void finalize_kernel(const double* __restrict__ sums, const int* __restrict__ wcnt,
                                                       const float* __restrict__ c_old, float* __restrict__ c_new,
                                                       double* __restrict__ shift, int32_t* __restrict__ counts, int D) {
  __shared__ double sh[2];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int n = wcnt[k];
  const double alpha = n > 0 ? 1.0 / (double)n : 1.0;  // an empty cluster keeps its sum (0 unless a relocation emptied it)
  double acc = 0.0;
  for (int d = tid; d < D; d += 128) {
    const float v = (float)(sums[(long)k * D + d] * alpha);
    c_new[(long)k * D + d] = v;
    const double df = (double)v - (double)c_old[(long)k * D + d];
    acc += df * df;
  }
  acc = block_sum<kSequential, false>(acc, sh);
  if (tid == 0) {
    shift[k] = sqrt(acc);
    if (counts) counts[k] = n;
  }
}

// flags[0] verdict (0 go on, 1 labels unchanged, 2 center_shift_tot <= tol), [1] labels changed, [2] empty clusters before
// relocation, [3] clusters relocated; stats[0] center_shift_tot
__global__ __launch_bounds__(256) void verdict_kernel(const double* __restrict__ shift, const int* __restrict__ state,
                                                      int32_t* __restrict__ flags, double* __restrict__ stats, int K, double tol) {
  __shared__ double sh[4];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int k = tid; k < K; k += 256) s += shift[k] * shift[k];
  const double tot = block_sum<kSequential, false>(s, sh);
  if (tid == 0) {
    const int changed = state[0];
    flags[0] = !changed ? 1 : (tot <= tol ? 2 : 0);
    flags[1] = changed;
    flags[2] = state[1];
    flags[3] = state[3];
    stats[0] = tot;
  }
}

// out[0] = sum_r dist[r], per thread in row order, then the waves' butterflies, then the waves in order
__global__ __launch_bounds__(1024) void sum_kernel(const double* __restrict__ v, double* __restrict__ out, long n) {
  __shared__ double sh[16];
  const int tid = threadIdx.x;
  const long per = (n + 1023) / 1024, lo = min(n, tid * per), hi = min(n, lo + per);
  double s = 0.0;
  for (long i = lo; i < hi; ++i) s += v[i];
  s = block_sum<kSequential, false>(s, sh);  // no wave total is -0.0: s starts at +0.0 and only adds
  if (tid == 0) out[0] = s;
}

// ---------------------------------------------------------------------------------------------------- EMA codebook
// Steps 1-3 of the update (include/alvq.h): cs = decay cs + (1 - decay) c; n = sum_k cs in fp64 (per thread in code order,
// the wave butterflies, the waves in order); cs = (cs + eps) / (n + K eps) n.  The unsmoothed value is recomputed in the
// second pass instead of being kept (K <= 16384 doubles would not fit LDS).  Nothing is written when *skip != 0.
__global__ __launch_bounds__(1024) void ema_size_kernel(const float* __restrict__ counts, float* __restrict__ cs, const float* skip,
                                                        int K, double decay, double eps) {
  __shared__ double sh[16];
  if (skip && *skip != 0.f) return;
  const int tid = threadIdx.x;
  const double omd = 1.0 - decay;
  double s = 0.0;
  for (int k = tid; k < K; k += 1024) s += decay * (double)cs[k] + omd * (double)counts[k];
  const double n = block_sum<kSequential, false>(s, sh);  // no wave total is -0.0: s starts at +0.0 and only adds
  const double den = n + (double)K * eps;
  for (int k = tid; k < K; k += 1024) {
    const double v = decay * (double)cs[k] + omd * (double)counts[k];
    cs[k] = (float)((v + eps) / den * n);
  }
}

// Steps 4-5: W = decay W + (1 - decay) s (fp64, rounded once); E = W / cs (fp32).  Nothing is written when *skip != 0.
__global__ __launch_bounds__(256) void ema_apply_kernel(const float* __restrict__ sums, const float* __restrict__ cs,
                                                        float* __restrict__ W, float* __restrict__ E, const float* skip, long n,
                                                        int D, double decay) {
  if (skip && *skip != 0.f) return;
  const double omd = 1.0 - decay;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    const float w = (float)(decay * (double)W[e] + omd * (double)sums[e]);
    W[e] = w;
    E[e] = w / cs[e / D];
  }
}

// ---------------------------------------------------------------------------------------------------- column statistics
// part[g][d] = sum over rows of chunk g of x (mode 0) or of (x - mean[d])^2 (mode 1), in fp64, in row order
__global__ __launch_bounds__(128) void colsum_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                                     double* __restrict__ part, long N, int D, int mode) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const long r0 = (long)g * KM_CS_ROWS, r1 = min(N, r0 + KM_CS_ROWS);
  for (int d = tid; d < D; d += 128) {
    const double m = mode ? mean[d] : 0.0;
    double s = 0.0;
    for (long r = r0; r < r1; ++r) {
      const double v = (double)x[r * D + d] - m;
      s += mode ? v * v : v;
    }
    part[(long)g * D + d] = s;
  }
}

// mode 0: mean[d] (fp64) and mean32[d] = fl32(mean[d]);  mode 1: var_mean[0] = (sum_d var[d]) / D, var[d] = sum / N
__global__ __launch_bounds__(512) void colreduce_kernel(const double* __restrict__ part, double* __restrict__ mean,
                                                        float* __restrict__ mean32, double* __restrict__ var_mean, long N, int D,
                                                        int G, int mode) {
  __shared__ double col[KM_MAX_D];
  const int d = threadIdx.x;
  if (d < D) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(long)g * D + d];
    s /= (double)N;
    if (mode == 0) {
      mean[d] = s;
      mean32[d] = (float)s;
    } else {
      col[d] = s;
    }
  }
  __syncthreads();
  if (mode == 1 && d == 0) {
    double t = 0.0;
    for (int i = 0; i < D; ++i) t += col[i];
    var_mean[0] = t / (double)D;
  }
}

__global__ __launch_bounds__(256) void add_rows_kernel(const float* __restrict__ x, const float* __restrict__ v, float* __restrict__ y,
                                                       long n, int D, float alpha) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) y[e] = x[e] + alpha * v[e % D];
}

// ---------------------------------------------------------------------------------------------------- k-means++
struct PPState {
  double pot;       // current_pot
  int64_t best;     // candidate slot of the last round's pick
  int64_t cand[PP_MAX_T];
};

// round c >= 1: r_t = u[c-1][t] * pot; candidate t = the first row whose blocked inclusive cumsum of closest_dist_sq is
// >= r_t (block prefixes over the per-block sums, then a wave scan inside the block), N - 1 when none is (np.clip)
__global__ __launch_bounds__(1024) void pick_kernel(const double* __restrict__ u, const double* __restrict__ dist_prev,
                                                    const double* __restrict__ part_prev, PPState* st, long N, int NBK, int T,
                                                    int c, long first) {
  __shared__ double shd[16];
  __shared__ int minb[PP_MAX_T];
  __shared__ double bex[PP_MAX_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (c == 0) {
    if (tid == 0) st->cand[0] = first;
    return;
  }
  const int best = (int)st->best;
  const double pot = st->pot;
  const double* closest = dist_prev + (long)best * N;
  const double* blk = part_prev + (long)best * NBK;
  if (tid < PP_MAX_T) minb[tid] = 0x7fffffff;
  const int per = (NBK + 1023) / 1024;
  const int lo = min(NBK, tid * per), hi = min(NBK, lo + per);
  double s = 0.0;
  for (int b = lo; b < hi; ++b) s += blk[b];
  double run = block_scan_excl_f64(s, shd);
  double r[PP_MAX_T];
  int found[PP_MAX_T];
  double fex[PP_MAX_T];
#pragma unroll
  for (int t = 0; t < PP_MAX_T; ++t) {
    r[t] = t < T ? u[(long)(c - 1) * T + t] * pot : 0.0;
    found[t] = 0x7fffffff;
    fex[t] = 0.0;
  }
  for (int b = lo; b < hi; ++b) {
    const double nxt = run + blk[b];
#pragma unroll
    for (int t = 0; t < PP_MAX_T; ++t)
      if (t < T && found[t] == 0x7fffffff && nxt >= r[t]) {
        found[t] = b;
        fex[t] = run;
      }
    run = nxt;
  }
#pragma unroll
  for (int t = 0; t < PP_MAX_T; ++t)
    if (t < T && found[t] != 0x7fffffff) atomicMin(&minb[t], found[t]);  // integer min: the same result in any order
  __syncthreads();
#pragma unroll
  for (int t = 0; t < PP_MAX_T; ++t)
    if (t < T && found[t] != 0x7fffffff && found[t] == minb[t]) bex[t] = fex[t];  // one thread: the ranges are disjoint
  __syncthreads();
  if (wave >= T) return;
  const int b = minb[wave];
  long id = N - 1;
  if (b != 0x7fffffff) {
    const long row = (long)b * PP_ROWS + lane;
    const double v = row < N ? closest[row] : 0.0;
    const double inc = wave_scan_incl(v);
    const bool hit = row < N && bex[wave] + inc >= r[wave];
    const unsigned long long m = __ballot(hit);
    id = m ? (long)b * PP_ROWS + (__ffsll(m) - 1) : min(N - 1, (long)b * PP_ROWS + PP_ROWS - 1);
  }
  if (lane == 0) st->cand[wave] = min(id, N - 1);
}

// dist[t][r] = min(closest[r], |x_r - x_cand_t|^2) (round 0: the distance itself), part[t][blk] = its sum over the block's rows
__global__ __launch_bounds__(256) void ppdist_kernel(const float* __restrict__ x, const double* __restrict__ dist_prev,
                                                     double* __restrict__ dist, double* __restrict__ part, const PPState* st,
                                                     long N, int D, int NBK, int T, int c) {
  __shared__ float xs[PP_ROWS][PP_DC + 4];
  __shared__ float cs[PP_MAX_T][PP_DC];
  __shared__ double sh[4][PP_MAX_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = tid >> 2, q = tid & 3;
  const long r0 = (long)blockIdx.x * PP_ROWS;
  double acc[PP_MAX_T] = {};
  for (int d0 = 0; d0 < D; d0 += PP_DC) {
    for (int e = tid; e < PP_ROWS * PP_DC; e += 256) {
      const int rr = e / PP_DC, dd = e % PP_DC;
      const long r = r0 + rr;
      xs[rr][dd] = (r < N && d0 + dd < D) ? x[r * D + d0 + dd] : 0.0f;
    }
    for (int e = tid; e < T * PP_DC; e += 256) {
      const int t = e / PP_DC, dd = e % PP_DC;
      cs[t][dd] = d0 + dd < D ? x[st->cand[t] * D + d0 + dd] : 0.0f;
    }
    __syncthreads();
    for (int j = 0; j < PP_DC / 4; ++j) {
      const int dd = q + 4 * j;
      const double xv = (double)xs[row][dd];
#pragma unroll
      for (int t = 0; t < PP_MAX_T; ++t)
        if (t < T) {
          const double df = xv - (double)cs[t][dd];
          acc[t] += df * df;
        }
    }
    __syncthreads();
  }
  const long r = r0 + row;
  const double* closest = c > 0 ? dist_prev + st->best * N : nullptr;
  const double cl = (closest && r < N) ? closest[r] : 0.0;
#pragma unroll
  for (int t = 0; t < PP_MAX_T; ++t) {
    if (t >= T) continue;  // T is uniform over the workgroup
    double a = acc[t];
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    const double m = closest ? fmin(cl, a) : a;
    if (q == 0 && r < N) dist[(long)t * N + r] = m;
    const double bs = wave_sum_lane0((q == 0 && r < N) ? m : 0.0);
    if (lane == 0) sh[wave][t] = bs;
  }
  __syncthreads();
  if (tid < T) part[(long)tid * NBK + blockIdx.x] = combine_waves<4, kSequential, PP_MAX_T>(&sh[0][tid]);
}

// pot_t = sum of part[t][.] in block order; the least (lowest t on ties) is round c's centre
__global__ __launch_bounds__(1024) void select_kernel(const float* __restrict__ x, const double* __restrict__ part, PPState* st,
                                                      float* __restrict__ centers, int64_t* __restrict__ indices, int NBK, int D,
                                                      int T, int c) {
  __shared__ double sh[PP_MAX_T][16];
  __shared__ long pick;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int t = 0; t < T; ++t) {
    double s = 0.0;
    for (int b = tid; b < NBK; b += 1024) s += part[(long)t * NBK + b];
    s = wave_sum_lane0(s);
    if (lane == 0) sh[t][wave] = s;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    double bp = 0.0;
    for (int t = 0; t < T; ++t) {
      const double p = combine_waves<16, kSequential>(sh[t]);  // no wave total is -0.0: s starts at +0.0 and only adds
      if (t == 0 || p < bp) {
        bp = p;
        best = t;
      }
    }
    st->best = best;
    st->pot = bp;
    pick = st->cand[best];
    indices[c] = pick;
  }
  __syncthreads();
  for (int d = tid; d < D; d += 1024) centers[(long)c * D + d] = x[pick * D + d];
}

}  // namespace alvq

using namespace alvq;

static int km_grid(long items, int per_block, int cap = 4096) {
  long g = (items + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

static int km_check(int64_t N, int K, int D, const char* who) {
  ALVQ_REQUIRE(N > 0 && K > 0 && D > 0, ALVQ_EINVAL, "%s: bad dims N=%ld K=%d D=%d", who, (long)N, K, D);
  ALVQ_REQUIRE(N < (1L << 30), ALVQ_EUNSUPPORTED, "%s: N=%ld >= 2^30", who, (long)N);
  ALVQ_REQUIRE(K <= KM_MAX_K, ALVQ_EUNSUPPORTED, "%s: K=%d > %d", who, K, KM_MAX_K);
  ALVQ_REQUIRE(D <= KM_MAX_D, ALVQ_EUNSUPPORTED, "%s: D=%d > %d", who, D, KM_MAX_D);
  return 0;
}

struct UpdateWs {
  double *part, *sums, *dist, *shift;
  int *HO, *rank, *perm, *blk_changed, *start, *cnt, *wcnt, *seg_start, *elist, *state;
};

// carves a workspace into 256-byte aligned pieces; with a null base it only sizes (every piece null, off = the bytes needed)
struct Carver {
  char* base;
  int64_t off = 0;
  template <typename T>
  void take(T*& p, int64_t count) {
    p = base ? (T*)(base + off) : nullptr;
    off += (count * (int64_t)sizeof(T) + 255) / 256 * 256;
  }
};

static int64_t update_layout(int64_t N, int K, int D, char* base, UpdateWs* w) {
  const int64_t NB = (N + KM_SB - 1) / KM_SB, NS = (N + KM_SEG - 1) / KM_SEG + K;
  Carver c{base};
  UpdateWs v;
  c.take(v.part, NS * D);
  c.take(v.sums, (int64_t)K * D);
  c.take(v.dist, N);
  c.take(v.shift, K);
  c.take(v.HO, (int64_t)K * NB);
  c.take(v.rank, N);
  c.take(v.perm, N);
  c.take(v.blk_changed, NB);
  c.take(v.start, K);
  c.take(v.cnt, K);
  c.take(v.wcnt, K);
  c.take(v.seg_start, K + 1);
  c.take(v.elist, K);
  c.take(v.state, 8);
  if (w) *w = v;
  return c.off;
}

// the sort by label and the fp64 segment sums that the Lloyd update and the EMA statistics share: hist .. segsum
static void launch_sorted_segsums(const float* x, const int64_t* labels, const int64_t* labels_old, const UpdateWs& w, int64_t N,
                                  int K, int D, hipStream_t s) {
  const int nb = (int)((N + KM_SB - 1) / KM_SB);
  hipLaunchKernelGGL(hist_kernel, dim3(nb), dim3(64), (size_t)K * sizeof(int), s, labels, labels_old, w.HO, w.rank,
                     w.blk_changed, (long)N, K, nb);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.HO, w.blk_changed, w.start, w.cnt, w.seg_start, w.state, K, nb);
  hipLaunchKernelGGL(scatter_kernel, dim3(km_grid(N, 256)), dim3(256), 0, s, labels, w.HO, w.rank, w.perm, (long)N, K, nb);
  const int nseg_max = (int)((N + KM_SEG - 1) / KM_SEG + K);
  hipLaunchKernelGGL(segsum_kernel, dim3(nseg_max), dim3(128), 0, s, x, w.perm, w.start, w.cnt, w.seg_start, w.state, w.part, K, D);
}

extern "C" int64_t alvq_kmeans_update_workspace_bytes(int64_t N, int K, int D) {
  if (N <= 0 || K <= 0 || D <= 0 || N >= (1L << 30) || K > KM_MAX_K || D > KM_MAX_D) return -1;
  if ((int64_t)K * ((N + KM_SB - 1) / KM_SB) >= (1L << 31)) return -1;
  return update_layout(N, K, D, nullptr, nullptr);
}

extern "C" int alvq_kmeans_update_f32(const float* x, const int64_t* labels, const int64_t* labels_old, const float* centers_old,
                                      float* centers_new, int32_t* counts, double* stats, int32_t* flags, void* workspace,
                                      int64_t N, int K, int D, double tol, void* stream) {
  const char* who = "alvq_kmeans_update_f32";
  ALVQ_REQUIRE(x && labels && centers_old && centers_new && stats && flags && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  if (int rc = km_check(N, K, D, who)) return rc;
  ALVQ_REQUIRE(centers_old != centers_new, ALVQ_EINVAL, "%s: centers_new must not alias centers_old", who);
  const int64_t NB = (N + KM_SB - 1) / KM_SB;
  ALVQ_REQUIRE((int64_t)K * NB < (1L << 31), ALVQ_EUNSUPPORTED, "%s: K * N / %d too large", who, KM_SB);
  hipStream_t s = (hipStream_t)stream;
  UpdateWs w;
  update_layout(N, K, D, (char*)workspace, &w);
  launch_sorted_segsums(x, labels, labels_old, w, N, K, D, s);
  hipLaunchKernelGGL((clustersum_kernel<double, int>), dim3(K), dim3(128), 0, s, w.part, w.seg_start, w.cnt, w.sums, w.wcnt, D);
  hipLaunchKernelGGL(rowdist_kernel, dim3(km_grid(N, 4, 2048)), dim3(256), 0, s, x, labels, centers_old, w.dist,
                     (const int*)(w.state + 1), (long)N, K, D);
  hipLaunchKernelGGL(relocate_kernel, dim3(1), dim3(1024), 0, s, x, labels, w.dist, w.sums, w.wcnt, w.elist, w.state, (long)N, K, D);
  hipLaunchKernelGGL(finalize_kernel, dim3(K), dim3(128), 0, s, w.sums, w.wcnt, centers_old, centers_new, w.shift, counts, D);
  hipLaunchKernelGGL(verdict_kernel, dim3(1), dim3(256), 0, s, w.shift, w.state, flags, stats, K, tol);
  return check_launch(who);
}

// EMA statistics: the Lloyd update's sort and fp64 cluster sums (the same layout and launches up to clustersum), written as
// fp32 counts / sums into the caller's buffers.  Counts are exact in fp32 below 2^24 rows.
extern "C" int64_t alvq_vq_ema_stats_workspace_bytes(int64_t N, int K, int D) {
  if (N <= 0 || K <= 0 || D <= 0 || N >= (1L << 24) || K > KM_MAX_K || D > KM_MAX_D) return -1;
  return update_layout(N, K, D, nullptr, nullptr);
}

extern "C" int alvq_vq_ema_stats_f32(const float* x, const int64_t* idx, float* counts, float* sums, void* workspace, int64_t N,
                                     int K, int D, void* stream) {
  const char* who = "alvq_vq_ema_stats_f32";
  ALVQ_REQUIRE(x && idx && counts && sums && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  if (int rc = km_check(N, K, D, who)) return rc;
  ALVQ_REQUIRE(N < (1L << 24), ALVQ_EUNSUPPORTED, "%s: N=%ld >= 2^24 rows (counts travel as fp32)", who, (long)N);
  hipStream_t s = (hipStream_t)stream;
  UpdateWs w;
  update_layout(N, K, D, (char*)workspace, &w);
  launch_sorted_segsums(x, idx, nullptr, w, N, K, D, s);
  hipLaunchKernelGGL((clustersum_kernel<float, float>), dim3(K), dim3(128), 0, s, w.part, w.seg_start, w.cnt, sums, counts, D);
  return check_launch(who);
}

extern "C" int alvq_vq_ema_update_f32(const float* counts, const float* sums, float* cluster_size, float* ema_w, float* codebook,
                                      const float* skip, int K, int D, double decay, double epsilon, void* stream) {
  const char* who = "alvq_vq_ema_update_f32";
  ALVQ_REQUIRE(counts && sums && cluster_size && ema_w && codebook, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(K > 0 && D > 0, ALVQ_EINVAL, "%s: bad dims K=%d D=%d", who, K, D);
  ALVQ_REQUIRE(K <= KM_MAX_K && D <= KM_MAX_D, ALVQ_EUNSUPPORTED, "%s: K=%d D=%d outside K <= %d, D <= %d", who, K, D, KM_MAX_K,
               KM_MAX_D);
  ALVQ_REQUIRE(decay > 0.0 && decay < 1.0 && epsilon > 0.0, ALVQ_EINVAL, "%s: decay=%g outside (0, 1) or epsilon=%g <= 0", who,
               decay, epsilon);
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)K * D;
  hipLaunchKernelGGL(ema_size_kernel, dim3(1), dim3(1024), 0, s, counts, cluster_size, skip, K, decay, epsilon);
  hipLaunchKernelGGL(ema_apply_kernel, dim3(km_grid(n, 256, 1024)), dim3(256), 0, s, sums, (const float*)cluster_size, ema_w,
                     codebook, skip, n, D, decay);
  return check_launch(who);
}

extern "C" int64_t alvq_kmeans_inertia_workspace_bytes(int64_t N) {
  if (N <= 0 || N >= (1L << 30)) return -1;
  return N * (int64_t)sizeof(double);
}

extern "C" int alvq_kmeans_inertia_f32(const float* x, const int64_t* labels, const float* centers, double* inertia, void* workspace,
                                       int64_t N, int K, int D, void* stream) {
  const char* who = "alvq_kmeans_inertia_f32";
  ALVQ_REQUIRE(x && labels && centers && inertia && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  if (int rc = km_check(N, K, D, who)) return rc;
  hipStream_t s = (hipStream_t)stream;
  double* dist = (double*)workspace;
  hipLaunchKernelGGL(rowdist_kernel, dim3(km_grid(N, 4, 2048)), dim3(256), 0, s, x, labels, centers, dist, (const int*)nullptr,
                     (long)N, K, D);
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(1024), 0, s, dist, inertia, (long)N);
  return check_launch(who);
}

extern "C" int64_t alvq_kmeans_col_stats_workspace_bytes(int64_t N, int D) {
  if (N <= 0 || N >= (1L << 30) || D <= 0 || D > KM_MAX_D) return -1;
  return (((N + KM_CS_ROWS - 1) / KM_CS_ROWS) * D + D) * (int64_t)sizeof(double);
}

extern "C" int alvq_kmeans_col_stats_f32(const float* x, float* mean, double* var_mean, void* workspace, int64_t N, int D,
                                         void* stream) {
  const char* who = "alvq_kmeans_col_stats_f32";
  ALVQ_REQUIRE(x && mean && var_mean && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  if (int rc = km_check(N, 1, D, who)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int G = (int)((N + KM_CS_ROWS - 1) / KM_CS_ROWS);
  double* part = (double*)workspace;
  double* mean64 = part + (int64_t)G * D;
  hipLaunchKernelGGL(colsum_kernel, dim3(G), dim3(128), 0, s, x, (const double*)nullptr, part, (long)N, D, 0);
  hipLaunchKernelGGL(colreduce_kernel, dim3(1), dim3(512), 0, s, part, mean64, mean, var_mean, (long)N, D, G, 0);
  hipLaunchKernelGGL(colsum_kernel, dim3(G), dim3(128), 0, s, x, (const double*)mean64, part, (long)N, D, 1);
  hipLaunchKernelGGL(colreduce_kernel, dim3(1), dim3(512), 0, s, part, mean64, mean, var_mean, (long)N, D, G, 1);
  return check_launch(who);
}

extern "C" int alvq_kmeans_add_rows_f32(const float* x, const float* v, float* y, int64_t N, int D, float alpha, void* stream) {
  const char* who = "alvq_kmeans_add_rows_f32";
  ALVQ_REQUIRE(x && v && y, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(N > 0 && D > 0, ALVQ_EINVAL, "%s: bad dims N=%ld D=%d", who, (long)N, D);
  hipLaunchKernelGGL(add_rows_kernel, dim3(km_grid(N * D, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, v, y, (long)(N * D), D,
                     alpha);
  return check_launch(who);
}

static int64_t pp_layout(int64_t N, int T, char* base, double** dist, double** part, PPState** st) {
  const int64_t NBK = (N + PP_ROWS - 1) / PP_ROWS;
  Carver c{base};
  for (int i = 0; i < 2; ++i) c.take(dist[i], (int64_t)T * N);
  for (int i = 0; i < 2; ++i) c.take(part[i], (int64_t)T * NBK);
  c.take(*st, 1);
  return c.off;
}

extern "C" int64_t alvq_kmeans_plusplus_workspace_bytes(int64_t N, int T) {
  if (N <= 0 || N >= (1L << 30) || T < 1 || T > PP_MAX_T) return -1;
  double* d[2];
  double* p[2];
  PPState* st;
  return pp_layout(N, T, nullptr, d, p, &st);
}

extern "C" int alvq_kmeans_plusplus_f32(const float* x, const double* uniforms, float* centers, int64_t* indices, void* workspace,
                                        int64_t N, int K, int D, int T, int64_t first, void* stream) {
  const char* who = "alvq_kmeans_plusplus_f32";
  ALVQ_REQUIRE(x && centers && indices && workspace && (uniforms || K == 1), ALVQ_EINVAL, "%s: null pointer", who);
  if (int rc = km_check(N, K, D, who)) return rc;
  ALVQ_REQUIRE(K <= N, ALVQ_EINVAL, "%s: K=%d > N=%ld", who, K, (long)N);
  ALVQ_REQUIRE(T >= 1 && T <= PP_MAX_T, ALVQ_EUNSUPPORTED, "%s: T=%d outside [1, %d]", who, T, PP_MAX_T);
  ALVQ_REQUIRE(first >= 0 && first < N, ALVQ_EINVAL, "%s: first=%ld outside [0, N)", who, (long)first);
  hipStream_t s = (hipStream_t)stream;
  double* dist[2];
  double* part[2];
  PPState* st;
  pp_layout(N, T, (char*)workspace, dist, part, &st);
  const int NBK = (int)((N + PP_ROWS - 1) / PP_ROWS);
  for (int c = 0; c < K; ++c) {
    const int cur = c & 1, prev = cur ^ 1, t = c == 0 ? 1 : T;
    hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(1024), 0, s, uniforms, dist[prev], part[prev], st, (long)N, NBK, T, c, (long)first);
    hipLaunchKernelGGL(ppdist_kernel, dim3(NBK), dim3(256), 0, s, x, dist[prev], dist[cur], part[cur], st, (long)N, D, NBK, t, c);
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(1024), 0, s, x, part[cur], st, centers, indices, NBK, D, t, c);
    if (int rc = check_launch(who)) return rc;
  }
  return ALVQ_OK;
}
