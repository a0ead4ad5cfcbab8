// ILRMA blind source separation of a microphone array's complex spectrograms: independent low-rank matrix analysis (Kitamura,
// Ono, Sawada, Kameoka, Saruwatari, IEEE/ACM TASLP 2016), AuxIVA's iterative projection with a rank-L non-negative model of every
// source's variance, fitted by multiplicative updates between the demixing updates.  The definitions are the comment on
// alvq_ilrma_* in include/alvq.h; tests/helpers/ilrma_ref.py restates them in numpy.  All arithmetic is float64; only Y is rounded.
// The bin check, the weighted covariances, the elimination and the projection are AuxIVA's, from csrc/iva_kernels.h.
//
// Before the first iteration:
// iva_check_kernel<R>        AuxIVA's status and the start of W.
// ilrma_item_kernel          a workgroup an item: activations0 -> activations, and a flag for an item whose activations0 hold a
//                            value that is not finite or not > 0 (__syncthreads_or: an OR has no order).
// ilrma_bin_kernel           a wave a bin: basis0 -> basis for the bin's D L values; a value that is not finite or not > 0, or
//                            the item's flag, gives the bin status 1 and W = I.
// One iteration:
// ilrma_power_kernel<R, D>   step 1.  A wave a pair (bin, k) as in iva_cov_kernel, so that the D waves of a bin read the same
//                            rows of X from cache; row k of W by uniform loads; lane l takes the frames t = l, l + 64, ...,
//                            stores P (B, D, F, T) and adds it to one accumulator; wave_sum; lane 0 stores the row's sum.
// ilrma_lambda_kernel        a wave a pair (b, k): 64 row sums a load, lane j's added in the order of j (v_readlane), so that
//                            the chain is f rising over the bins whose status is not 1, the same in every lane; their number;
//                            lam.  (A thread a pair with one load an addition took 20 us at F = 201, 201 load latencies in a
//                            row; the same chain fed by __shfl, which goes through the LDS crossbar, 14 us.)
// ilrma_basis_kernel<L>      steps 2 and 3.  A wave a row (b, k, f): the row's L basis values are uniform and are normalised as
//                            they are loaded; lane l takes the frames t = l, l + 64, ... rising with the L activations of a
//                            frame in registers and 2 L accumulators, which meet in wave_sum's butterfly; lane l stores entry l.
// ilrma_act_kernel<L>        step 4.  The grid runs over (frame tiles of 64, b), a workgroup has D waves, wave k owns source k
//                            and a lane a frame, as in iva_activity_kernel.  The frame's L activations and its 2 L accumulators
//                            sit in registers; it walks f rising, the bin's L basis values come by uniform loads, and a bin of
//                            status 1 is loaded and dropped, so that the loop has no branch and several bins' loads are in flight.
// ilrma_weight_kernel<L>     step 5's weights: 1 / R over P, in the bins of status 0, a wave a row as in ilrma_basis_kernel.
// iva_cov_kernel<R, D>       with the weights of its own bin (bin_stride = T).
// iva_solve_kernel<D, true>  with row k of W divided by sqrt(lam[k]) as it is loaded: step 2's share of W.
// After the last iteration: iva_project_kernel<R, D>.
// ONE DIVERGENCE from the suggested plan: the weights 1 / R of step 5 have a launch of their own that writes them over P,
// 8 B D F T bytes written and read once more, and the covariance takes them by a stride.  Computed inside iva_cov_kernel they
// would make that kernel a template of L as well -- 2 x 8 x 16 instantiations of the largest kernel here -- and put L loads and
// a division between the loads of a frame and its D^2 fused multiply-adds.  Nothing has been measured that says otherwise.
// v_mfma_f64 is not used, for the reason csrc/wpe.hip gives.  No atomics, no host-side decision between the launches.
// Every grid over rows, pairs or bins is capped at kMaxBlocks workgroups and strides, whole waves at a time.
// What the launches cost: DESIGN.md.
#include "iva_kernels.h"

namespace alvq {

constexpr int ILRMA_MAX_L = 16;            // 2 L accumulators and L values a lane: 96 VGPRs at the cap, 182 with the rest

// max(v, floor) that also sends a value that is not finite (a NaN included) to floor
__device__ __forceinline__ double ilrma_floor(double v, double floor) { return (v > floor && v <= DBL_MAX) ? v : floor; }
__device__ __forceinline__ bool ilrma_positive(double v) { return v > 0.0 && v <= DBL_MAX; }

// R of a frame and bin: floor(sum_l bs[l] a[l]), l rising from the first product, every product rounded
template <int L>
__device__ __forceinline__ double ilrma_model(const double (&bs)[L], const double (&a)[L], double floor) {
  double r = bs[0] * a[0];
#pragma unroll
  for (int l = 1; l < L; ++l) r += bs[l] * a[l];
  return ilrma_floor(r, floor);
}

// the multiplicative update of one entry: v sqrt(num / den) where the ratio is finite, v where it is not; floored
__device__ __forceinline__ double ilrma_update(double v, double num, double den, double floor) {
  const double ratio = num / den;
  return ilrma_floor(is_finite(ratio) ? v * sqrt(ratio) : v, floor);
}

// -------------------------------------------------------------------------------------------------------------------- start
__global__ __launch_bounds__(IVA_THREADS) void ilrma_item_kernel(const double* A0, double* A, int* item_bad, long n) {
  const double* src = A0 + (long)blockIdx.x * n;
  double* dst = A + (long)blockIdx.x * n;
  int bad = 0;
  for (long i = threadIdx.x; i < n; i += IVA_THREADS) {
    const double v = src[i];
    if (!ilrma_positive(v)) bad = 1;
    dst[i] = v;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) item_bad[blockIdx.x] = bad;
}

__global__ __launch_bounds__(IVA_THREADS) void ilrma_bin_kernel(const double* basis0, double* basis, const int* item_bad, double2* W,
                                                                int* status, long nbins, int D, int L, int F) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (long bin = (long)blockIdx.x * IVA_WAVES + wv; bin < nbins; bin += (long)gridDim.x * IVA_WAVES) {
    const int b = (int)(bin / F), f = (int)(bin % F);
    int bad = item_bad[b];
    for (int i = lane; i < D * L; i += kWave) {
      const int k = i / L, l = i - k * L;
      const long at = (((long)b * D + k) * F + f) * L + l;
      const double v = basis0[at];
      if (!ilrma_positive(v)) bad = 1;
      basis[at] = v;
    }
    bad = wave_or(bad);
    if (bad) {
      if (lane < D * D) W[bin * (D * D) + lane] = make_double2(lane / D == lane % D ? 1.0 : 0.0, 0.0);
      if (lane == 0) status[bin] = IVA_BAD_INPUT;
    }
  }
}

// -------------------------------------------------------------------------------------------------------------------- power
template <typename R, int D>
__global__ __launch_bounds__(IVA_THREADS) void ilrma_power_kernel(const void* X, const double2* W, const int* status, double* P,
                                                                  double* rowsum, long nbins, int F, int T) {
  typedef typename Cplx<R>::type C;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long chan_stride = (long)F * T;
  for (long e = (long)blockIdx.x * IVA_WAVES + wv; e < nbins * D; e += (long)gridDim.x * IVA_WAVES) {
    const long bin = e / D;
    const int k = (int)(e - bin * D);
    if (status[bin] == IVA_BAD_INPUT) continue;
    const int b = (int)(bin / F), f = (int)(bin % F);
    const C* xg = (const C*)X + ((long)b * D * F + f) * T;
    const long row = ((long)b * D + k) * F + f;
    double* prow = P + row * T;
    double2 w[D];
#pragma unroll
    for (int d = 0; d < D; ++d) w[d] = W[bin * (D * D) + k * D + d];
    double s = 0.0;
    for (int t = lane; t < T; t += kWave) {
      C v[D];
#pragma unroll
      for (int d = 0; d < D; ++d) v[d] = xg[d * chan_stride + t];
      double2 y = cmul(w[0], make_double2((double)v[0].x, (double)v[0].y));
#pragma unroll
      for (int d = 1; d < D; ++d) {
        const double2 q = cmul(w[d], make_double2((double)v[d].x, (double)v[d].y));
        y.x += q.x;
        y.y += q.y;
      }
      const double p = fma(y.y, y.y, y.x * y.x);
      prow[t] = p;
      s += p;
    }
    s = wave_sum(s);
    if (lane == 0) rowsum[row] = s;
  }
}

__global__ __launch_bounds__(IVA_THREADS) void ilrma_lambda_kernel(const double* rowsum, const int* status, double* lam, int pairs, int D,
                                                                   int F, int T) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * IVA_WAVES + (threadIdx.x >> 6);                      // a wave a pair: it leaves whole
  if (i >= pairs) return;
  const int* st = status + (long)(i / D) * F;
  const double* rs = rowsum + (long)i * F;
  double s = 0.0;
  int n = 0;
  for (int f0 = 0; f0 < F; f0 += kWave) {
    const int f = f0 + lane < F ? f0 + lane : F - 1;   // a lane past the row reads its last entry and is not counted
    const int live = f0 + lane < F && st[f] != IVA_BAD_INPUT;    // a row of a bin of status 1 was never written: loaded and dropped
    const double v = rs[f];
    const int lo = __double2loint(v), hi = __double2hiint(v);
#pragma unroll
    for (int j = 0; j < kWave; ++j) {                  // the 64 rows in the order of f, the same chain in every lane
      const double vj = __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
      const int lj = __builtin_amdgcn_readlane(live, j);
      s = lj ? s + vj : s;
      n += lj;
    }
  }
  const double l = s / ((double)n * (double)T);
  if (lane == 0) lam[i] = ilrma_positive(l) ? l : 1.0;
}

// -------------------------------------------------------------------------------------------------------------------- basis
template <int L>
__global__ __launch_bounds__(IVA_THREADS) void ilrma_basis_kernel(const double* P, const double* act, const double* lam, const int* status,
                                                                  double* basis, long rows, int D, int F, int T, double floor) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (long e = (long)blockIdx.x * IVA_WAVES + wv; e < rows; e += (long)gridDim.x * IVA_WAVES) {
    const long bk = e / F;
    const int f = (int)(e - bk * F);
    if (status[(bk / D) * F + f] == IVA_BAD_INPUT) continue;
    const double lm = lam[bk];
    double* brow = basis + e * L;
    const double* prow = P + e * T;
    const double* arow = act + bk * L * T;
    double bn[L], num[L], den[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      bn[l] = ilrma_floor(brow[l] / lm, floor);
      num[l] = 0.0;
      den[l] = 0.0;
    }
    for (int t = lane; t < T; t += kWave) {
      double a[L];
#pragma unroll
      for (int l = 0; l < L; ++l) a[l] = arow[(long)l * T + t];
      const double p = prow[t] / lm;
      const double inv = 1.0 / ilrma_model<L>(bn, a, floor);
      const double g = (p * inv) * inv;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        num[l] = fma(g, a[l], num[l]);
        den[l] = fma(inv, a[l], den[l]);
      }
    }
    double out = 0.0;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const double v = ilrma_update(bn[l], wave_sum(num[l]), wave_sum(den[l]), floor);
      if (lane == l) out = v;
    }
    if (lane < L) brow[lane] = out;
  }
}

// -------------------------------------------------------------------------------------------------------------- activations
template <int L>
__global__ __launch_bounds__(kWave * kMaxMics) void ilrma_act_kernel(const double* P, const double* basis, const double* lam,
                                                                      const int* status, double* act, int D, int F, int T,
                                                                      double floor) {
  const int lane = threadIdx.x & 63;
  const int k = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));          // wave k of the workgroup owns source k
  const int b = blockIdx.y, t = blockIdx.x * IVA_TILE + lane;
  const bool live = t < T;
  const int tt = live ? t : T - 1;                     // a lane past the row reads its last frame
  const long bk = (long)b * D + k;
  const double lm = lam[bk];
  double* acol = act + bk * L * T + tt;
  double a[L], num[L], den[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    a[l] = acol[(long)l * T];
    num[l] = 0.0;
    den[l] = 0.0;
  }
  const int* st = status + (long)b * F;
  constexpr int UNROLL = L <= 2 ? 8 : (L <= 4 ? 4 : 2);
#pragma unroll UNROLL
  for (int f = 0; f < F; ++f) {
    const bool skip = st[f] == IVA_BAD_INPUT;          // the same in every lane; what the bin holds is loaded and dropped
    const long row = bk * F + f;
    double bs[L];
#pragma unroll
    for (int l = 0; l < L; ++l) bs[l] = basis[row * L + l];
    const double p = P[row * T + tt] / lm;
    const double inv = 1.0 / ilrma_model<L>(bs, a, floor);
    const double g = (p * inv) * inv;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const double n = fma(g, bs[l], num[l]), d = fma(inv, bs[l], den[l]);
      num[l] = skip ? num[l] : n;
      den[l] = skip ? den[l] : d;
    }
  }
  if (live) {
#pragma unroll
    for (int l = 0; l < L; ++l) acol[(long)l * T] = ilrma_update(a[l], num[l], den[l], floor);
  }
}

// ------------------------------------------------------------------------------------------------------------------ weights
template <int L>
__global__ __launch_bounds__(IVA_THREADS) void ilrma_weight_kernel(const double* basis, const double* act, const int* status, double* P,
                                                                   long rows, int D, int F, int T, double floor) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (long e = (long)blockIdx.x * IVA_WAVES + wv; e < rows; e += (long)gridDim.x * IVA_WAVES) {
    const long bk = e / F;
    const int f = (int)(e - bk * F);
    if (status[(bk / D) * F + f] != 0) continue;
    const double* arow = act + bk * L * T;
    double bs[L];
#pragma unroll
    for (int l = 0; l < L; ++l) bs[l] = basis[e * L + l];
    for (int t = lane; t < T; t += kWave) {
      double a[L];
#pragma unroll
      for (int l = 0; l < L; ++l) a[l] = arow[(long)l * T + t];
      P[e * T + t] = 1.0 / ilrma_model<L>(bs, a, floor);
    }
  }
}

}  // namespace alvq

using namespace alvq;

#define ILRMA_FOR_L(L, CALL)  \
  switch (L) {                \
    case 1: CALL(1); break;   \
    case 2: CALL(2); break;   \
    case 3: CALL(3); break;   \
    case 4: CALL(4); break;   \
    case 5: CALL(5); break;   \
    case 6: CALL(6); break;   \
    case 7: CALL(7); break;   \
    case 8: CALL(8); break;   \
    case 9: CALL(9); break;   \
    case 10: CALL(10); break; \
    case 11: CALL(11); break; \
    case 12: CALL(12); break; \
    case 13: CALL(13); break; \
    case 14: CALL(14); break; \
    case 15: CALL(15); break; \
    default: CALL(16); break; \
  }

static int64_t ilrma_round16(int64_t n) { return (n + 15) / 16 * 16; }

static bool ilrma_dims_ok(int B, int D, int L, int F, int T) {
  return B >= 1 && B <= 65535 && F >= 1 && (long)B * F <= INT_MAX && D >= 1 && D <= kMaxMics && T >= 1 && T <= kMaxFrames && L >= 1 &&
         L <= ILRMA_MAX_L;
}

// the workspace, in this order: P (B, D, F, T) float64 (then 1 / R over it); V (B, F, D, D, D) complex128; the row sums of P
// (B, D, F); lam (B, D); the items' flags (B) int32
struct IlrmaWorkspace {
  int64_t p, v, rowsum, lam, flags, total;
  IlrmaWorkspace(int B, int D, int F, int T) {
    p = 0;
    v = p + ilrma_round16((int64_t)8 * B * D * F * T);
    rowsum = v + (int64_t)16 * B * F * D * D * D;
    lam = rowsum + ilrma_round16((int64_t)8 * B * D * F);
    flags = lam + ilrma_round16((int64_t)8 * B * D);
    total = flags + ilrma_round16((int64_t)4 * B);
  }
};

extern "C" int64_t alvq_ilrma_workspace_bytes(int B, int D, int L, int F, int T) {
  if (!ilrma_dims_ok(B, D, L, F, T)) return -1;
  return IlrmaWorkspace(B, D, F, T).total;
}

template <typename R>
static int ilrma_launch(const char* who, const R* X, const double* W0, const double* basis0, const double* activations0, double* W,
                        double* basis, double* activations, R* Y, int* status, void* workspace, int B, int D, int L, int F, int T,
                        int iterations, int ref, double floor, void* stream) {
  ALVQ_REQUIRE(X && basis0 && activations0 && W && basis && activations && Y && status && workspace, ALVQ_EINVAL, "%s: null pointer",
               who);
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_TRY(check_mics(who, D));
  ALVQ_TRY(check_frames(who, T));
  ALVQ_REQUIRE(L >= 1 && L <= ILRMA_MAX_L, ALVQ_EINVAL, "%s: L=%d (need 1 <= L <= 16)", who, L);
  ALVQ_REQUIRE(iterations >= 0 && iterations <= IVA_MAX_ITERATIONS, ALVQ_EINVAL, "%s: iterations=%d (need 0 <= iterations <= 256)", who,
               iterations);
  ALVQ_REQUIRE(ref >= 0 && ref < D, ALVQ_EINVAL, "%s: ref=%d (need 0 <= ref < D = %d)", who, ref, D);
  ALVQ_REQUIRE(std::isfinite(floor) && floor > 0.0, ALVQ_EINVAL, "%s: floor=%g must be finite and > 0", who, floor);
  const long nbins = (long)B * F, rows = nbins * D;
  hipStream_t s = (hipStream_t)stream;
  const IlrmaWorkspace ws(B, D, F, T);
  char* base = (char*)workspace;
  double* P = (double*)(base + ws.p);
  double2* V = (double2*)(base + ws.v);
  double* rowsum = (double*)(base + ws.rowsum);
  double* lam = (double*)(base + ws.lam);
  int* flags = (int*)(base + ws.flags);
  double2* Wd = (double2*)W;
  const dim3 threads(IVA_THREADS);
  const dim3 bin_grid = capped_grid((nbins + IVA_WAVES - 1) / IVA_WAVES), row_grid = capped_grid((rows + IVA_WAVES - 1) / IVA_WAVES);
  hipLaunchKernelGGL((iva_check_kernel<R>), bin_grid, threads, 0, s, (const void*)X, (const double2*)W0, Wd, status, nbins, D, F, T);
  hipLaunchKernelGGL(ilrma_item_kernel, dim3((unsigned)B), threads, 0, s, activations0, activations, flags, (long)D * L * T);
  hipLaunchKernelGGL(ilrma_bin_kernel, bin_grid, threads, 0, s, basis0, basis, (const int*)flags, Wd, status, nbins, D, L, F);
  const dim3 tiles((unsigned)((T + IVA_TILE - 1) / IVA_TILE), (unsigned)B);
  const int pairs = B * D;
  for (int it = 0; it < iterations; ++it) {
#define IVA_CALL(N)                                                                                                                 \
  hipLaunchKernelGGL((ilrma_power_kernel<R, N>), row_grid, threads, 0, s, (const void*)X, (const double2*)Wd, (const int*)status, P, \
                     rowsum, nbins, F, T)
    ALVQ_FOR_1_TO_8(D, IVA_CALL)
#undef IVA_CALL
    hipLaunchKernelGGL(ilrma_lambda_kernel, dim3((unsigned)((pairs + IVA_WAVES - 1) / IVA_WAVES)), threads, 0, s,
                       (const double*)rowsum, (const int*)status, lam, pairs, D, F, T);
#define ILRMA_CALL(N)                                                                                                          \
  hipLaunchKernelGGL((ilrma_basis_kernel<N>), row_grid, threads, 0, s, (const double*)P, (const double*)activations,            \
                     (const double*)lam, (const int*)status, basis, rows, D, F, T, floor)
    ILRMA_FOR_L(L, ILRMA_CALL)
#undef ILRMA_CALL
#define ILRMA_CALL(N)                                                                                                             \
  hipLaunchKernelGGL((ilrma_act_kernel<N>), tiles, dim3(kWave * D), 0, s, (const double*)P, (const double*)basis, (const double*)lam, \
                     (const int*)status, activations, D, F, T, floor)
    ILRMA_FOR_L(L, ILRMA_CALL)
#undef ILRMA_CALL
#define ILRMA_CALL(N)                                                                                                              \
  hipLaunchKernelGGL((ilrma_weight_kernel<N>), row_grid, threads, 0, s, (const double*)basis, (const double*)activations,            \
                     (const int*)status, P, rows, D, F, T, floor)
    ILRMA_FOR_L(L, ILRMA_CALL)
#undef ILRMA_CALL
#define IVA_CALL(N)                                                                                                                \
  hipLaunchKernelGGL((iva_cov_kernel<R, N>), row_grid, threads, 0, s, (const void*)X, (const double*)P, (const int*)status, V, nbins, \
                     F, T, (long)F * T, (long)T)
    ALVQ_FOR_1_TO_8(D, IVA_CALL)
#undef IVA_CALL
#define IVA_CALL(N) \
  hipLaunchKernelGGL((iva_solve_kernel<N, true>), bin_grid, threads, 0, s, (const double2*)V, Wd, status, nbins, (const double*)lam, F)
    ALVQ_FOR_1_TO_8(D, IVA_CALL)
#undef IVA_CALL
  }
#define IVA_CALL(N) \
  hipLaunchKernelGGL((iva_project_kernel<R, N>), capped_grid(nbins), threads, 0, s, (const void*)X, Wd, (void*)Y, status, nbins, F, T, ref)
  ALVQ_FOR_1_TO_8(D, IVA_CALL)
#undef IVA_CALL
  return check_launch(who);
}

extern "C" int alvq_ilrma_f32(const float* X, const double* W0, const double* basis0, const double* activations0, double* W,
                              double* basis, double* activations, float* Y, int* status, void* workspace, int B, int D, int L, int F,
                              int T, int iterations, int ref, double floor, void* stream) {
  return ilrma_launch("alvq_ilrma_f32", X, W0, basis0, activations0, W, basis, activations, Y, status, workspace, B, D, L, F, T,
                      iterations, ref, floor, stream);
}

extern "C" int alvq_ilrma_f64(const double* X, const double* W0, const double* basis0, const double* activations0, double* W,
                              double* basis, double* activations, double* Y, int* status, void* workspace, int B, int D, int L, int F,
                              int T, int iterations, int ref, double floor, void* stream) {
  return ilrma_launch("alvq_ilrma_f64", X, W0, basis0, activations0, W, basis, activations, Y, status, workspace, B, D, L, F, T,
                      iterations, ref, floor, stream);
}
