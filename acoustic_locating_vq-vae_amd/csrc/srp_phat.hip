// Source localisation from a microphone array's complex spectrograms: PHAT-weighted cross-spectra of the microphone pairs,
// GCC-PHAT at integer lags (Knapp, Carter 1976) and the SRP-PHAT map over candidate positions with its arg-max (DiBiase 2000).
// The definitions are the comment on alvq_phat_cross_spectra_* / alvq_gcc_phat_f64 / alvq_srp_phat_f64 in include/alvq.h;
// tests/helpers/srp_ref.py restates them in numpy.  All arithmetic is float64.
//
// phat_kernel        one workgroup of 256 threads a (b, f) bin.  The bin's D rows are turned into unit phasors once and kept
//                    in LDS (ROW_LDS: 16 D T bytes fit) or formed again from X at every use (the same function of the same
//                    values: the same bits).  A wave owns a pair: lane l adds t = l, l + 64, ... rising, wave_sum, / T.
// status_kernel      one workgroup an item: the OR over the item's psi band (a non-finite value, a non-zero value) and, for the
//                    map, over its microphone and candidate coordinates.  No atomics: wave_or, then the waves through LDS.
// gcc_kernel         a thread an output (b, p, l): the band rising, the angle reduced exactly as ((f l) mod n_fft) / n_fft.
// srp_map_kernel<D>  the hot loop, B x G x P x F_band rotations.  A workgroup of 512 threads owns an item and a tile of 512
//                    candidates, a thread a candidate.  The item's psi[:, band] sits in LDS as [f][p] (PSI_LDS: 16 P F_band
//                    bytes fit; 90 KB at P = 28 and 201 bins), so that every lane of a wave reads the same address: a broadcast,
//                    no bank conflicts; otherwise the same values are read from global memory (uniform addresses again).
//                    Rotations are formed per microphone, not per pair: D phasors z_d = e^{j pi x}, x = (2 f fs / n_fft) tau_d,
//                    per (candidate, bin), from csrc/steered_map.h's SteerWalk<D>: a rotation recurrence along f, re-anchored
//                    every K = 8 bins, which leaves at most 21 u on a phasor and 42 u on a pair term: the tests' bound
//                    carries + K for it next to its slack of 32.  The pair term is
//                    psi z_i conj(z_j), summed as  s_f = sum_i Re(z_i sum_{j > i} psi_ij conj(z_j))  with i and j rising: four
//                    fused multiply-adds per rotation (8 flops) and four more per microphone.  S = (sum_f w_f s_f) / (P W1) with
//                    f rising.  The order, the anchors included (they sit at f_lo + 8 n), depends on (D, f_lo, f_hi) alone, and a
//                    thread shares nothing with its neighbours: a candidate has the same bits alone or in any grid, an item
//                    alone or in any batch.  D is a template argument so that the phasors and the pair loops live in
//                    registers, fully unrolled.
// The arg-max is csrc/steered_map.h's map_peak_kernel<true, 256>; the status bits, the coordinate scan and the host rules of
// n_fft, the band, G, fs and c are that header's too.
// What the launches cost: DESIGN.md.
#include "steered_map.h"

namespace alvq {

constexpr int PHAT_THREADS = 256;
constexpr int PHAT_WAVES = PHAT_THREADS / kWave;
constexpr int PHAT_LDS_LIMIT = 160 * 1024 - 256;     // dynamic LDS: the 160 KiB less the static reduction scratch
constexpr int SRP_THREADS = 512;

__host__ __device__ inline int phat_pairs(int D) { return D * (D - 1) / 2; }

// z / |z| per component, 0 for z = 0; a non-finite component leaves a NaN
__device__ __forceinline__ double2 phat_unit(double re, double im) {
  const double h = hypot(re, im);
  if (h == 0.0) return make_double2(0.0, 0.0);
  return make_double2(re / h, im / h);
}

struct PhatArgs {
  const void* X;
  double2* psi;
  int B, D, F, T, f_lo, f_hi;
};

template <typename R, bool ROW_LDS>
__global__ __launch_bounds__(PHAT_THREADS) void phat_kernel(PhatArgs a) {
  typedef typename Cplx<R>::type C;
  extern __shared__ __attribute__((aligned(16))) unsigned char phat_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int D = a.D, T = a.T, P = phat_pairs(D);
  const long bin = blockIdx.x;
  const int b = (int)(bin / a.F), f = (int)(bin % a.F);
  double2* out = a.psi + (long)b * P * a.F + f;                          // pair p at out[p F]
  if (f < a.f_lo || f > a.f_hi) {                                        // the whole workgroup takes this branch or none of it
    for (int p = tid; p < P; p += PHAT_THREADS) out[(long)p * a.F] = make_double2(0.0, 0.0);
    return;
  }
  const long chan_stride = (long)a.F * T;
  const C* Xg = (const C*)a.X + ((long)b * D * a.F + f) * T;
  double2* us = (double2*)phat_smem;                                     // ROW_LDS: [D][T]

  auto unit = [&](int d, int t) -> double2 {
    if (ROW_LDS) return us[d * T + t];
    const C v = Xg[d * chan_stride + t];
    return phat_unit((double)v.x, (double)v.y);
  };

  if (ROW_LDS) {
    for (int e = tid; e < D * T; e += PHAT_THREADS) {
      const int d = e / T, t = e - d * T;
      const C v = Xg[d * chan_stride + t];
      us[e] = phat_unit((double)v.x, (double)v.y);
    }
    __syncthreads();
  }

  for (int p = wv; p < P; p += PHAT_WAVES) {
    int i = 0, rest = p;
    while (rest >= D - 1 - i) {                                          // lexicographic (i, j), i < j
      rest -= D - 1 - i;
      ++i;
    }
    const int j = i + 1 + rest;
    double2 acc = make_double2(0.0, 0.0);
    for (int t = lane; t < T; t += kWave) {
      const double2 x = unit(i, t), y = unit(j, t);
      acc.x += x.x * y.x + x.y * y.y;                                    // x conj(y)
      acc.y += x.y * y.x - x.x * y.y;
    }
    acc.x = wave_sum(acc.x);
    acc.y = wave_sum(acc.y);
    if (lane == 0) out[(long)p * a.F] = make_double2(acc.x / (double)T, acc.y / (double)T);
  }
}

// status[b] from the item's psi band and (mics != nullptr) its geometry
__global__ __launch_bounds__(PHAT_THREADS) void phat_status_kernel(const double2* psi, const double* mics, const double* cand,
                                                                    int* status, int P, int F, int f_lo, int f_hi, int D, int G,
                                                                    long mics_stride, long cand_stride) {
  __shared__ int s_flag[PHAT_WAVES];
  const int tid = threadIdx.x, b = blockIdx.x, Fb = f_hi - f_lo + 1;
  int seen = 0;                                                          // 1 non-finite psi, 2 non-zero psi, 4 bad coordinate
  const double2* row = psi + (long)b * P * F;
  for (int e = tid; e < P * Fb; e += PHAT_THREADS) {
    const int p = e / Fb, f = f_lo + (e - p * Fb);
    const double2 v = row[(long)p * F + f];
    if (!is_finite(v.x) || !is_finite(v.y)) seen |= 1;
    if (v.x != 0.0 || v.y != 0.0) seen |= 2;
  }
  if (mics) seen |= geometry_seen<PHAT_THREADS>(mics + (long)b * mics_stride, cand + (long)b * cand_stride, D, G, tid);
  seen = block_sum<kSequential, false, OpOr>(seen, s_flag);
  if (tid == 0) status[b] = map_status(seen);
}

__global__ __launch_bounds__(PHAT_THREADS) void gcc_kernel(const double2* psi, double* r, long total, int F, int n_fft, int L,
                                                            int f_lo, int f_hi, double W1) {
  const long idx = (long)blockIdx.x * PHAT_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int lags = 2 * L + 1;
  const long bp = idx / lags;
  const int l = (int)(idx - bp * lags) - L;
  const double2* row = psi + bp * F;
  double acc = 0.0;
  for (int f = f_lo; f <= f_hi; ++f) {
    long m = ((long)f * l) % n_fft;
    if (m < 0) m += n_fft;
    double s, c;
    sincospi((double)(2 * m) / (double)n_fft, &s, &c);
    const double2 v = row[f];
    const double w = (f == 0 || 2 * f == n_fft) ? 1.0 : 2.0;
    acc += w * (v.x * c - v.y * s);                                      // Re(psi e^{+j theta})
  }
  r[idx] = acc / W1;
}

struct SrpArgs {
  const double2* psi;
  const double* mics;
  const double* cand;
  double* map;
  const int* status;
  int B, G, F, n_fft, f_lo, f_hi;
  long mics_stride, cand_stride;
  double fs_over_n, c, norm;           // fs / n_fft;  the speed of sound;  P W1
};

template <int D, bool PSI_LDS>
__global__ __launch_bounds__(SRP_THREADS) void srp_map_kernel(SrpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char srp_smem[];
  constexpr int P = D * (D - 1) / 2;
  const int tid = threadIdx.x, b = blockIdx.y;
  const long g = (long)blockIdx.x * SRP_THREADS + tid;
  const int Fb = a.f_hi - a.f_lo + 1;
  double* out = a.map + (long)b * a.G;

  const int st = a.status[b];                                            // the same in every thread of the workgroup
  if (st) {
    if (g < a.G) out[g] = (st & (MAP_BAD_SPECTRUM | MAP_BAD_GEOMETRY)) ? __longlong_as_double(0x7ff8000000000000LL) : 0.0;
    return;
  }

  const double2* psig = a.psi + (long)b * P * a.F;
  double2* lds = (double2*)srp_smem;                                     // PSI_LDS: [Fb][P]
  if (PSI_LDS) {
    for (int e = tid; e < P * Fb; e += SRP_THREADS) {                    // consecutive threads read consecutive bins
      const int p = e / Fb, k = e - p * Fb;
      lds[k * P + p] = psig[(long)p * a.F + a.f_lo + k];
    }
    __syncthreads();
  }
  if (g >= a.G) return;

  SteerWalk<D> z(a.mics + (long)b * a.mics_stride, a.cand + (long)b * a.cand_stride + 3 * g, a.c, a.fs_over_n);
  double acc = 0.0;
  for (int k = 0; k < Fb; ++k) {
    const int f = a.f_lo + k;
    z.move(k, f, a.fs_over_n);
    const double2* row = PSI_LDS ? lds + k * P : psig + f;               // pair p at row[p] or row[p F]
    double s = 0.0;
    int p = 0;
#pragma unroll
    for (int i = 0; i < D - 1; ++i) {
      double cr = 0.0, ci = 0.0;                                         // sum_{j > i} psi_ij conj(z_j)
#pragma unroll
      for (int j = i + 1; j < D; ++j, ++p) {
        const double2 v = PSI_LDS ? row[p] : row[(long)p * a.F];
        cr = fma(v.x, z.zc[j], cr);
        cr = fma(v.y, z.zs[j], cr);
        ci = fma(v.y, z.zc[j], ci);
        ci = fma(-v.x, z.zs[j], ci);
      }
      s += fma(-z.zs[i], ci, z.zc[i] * cr);                              // Re(z_i (cr + j ci))
    }
    const double w = (f == 0 || 2 * f == a.n_fft) ? 1.0 : 2.0;
    acc = fma(w, s, acc);
  }
  out[g] = acc / a.norm;
}

}  // namespace alvq

using namespace alvq;

static int phat_check_band(const char* who, int B, int D, int F, int f_lo, int f_hi) {
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_TRY(check_mics(who, D, 2));
  return check_band(who, f_lo, f_hi, F);
}

// W1 = the sum of w_f over the band
static double phat_band_weight(int n_fft, int f_lo, int f_hi) {
  long w = 0;
  for (int f = f_lo; f <= f_hi; ++f) w += (f == 0 || 2 * f == n_fft) ? 1 : 2;
  return (double)w;
}

template <typename R>
static int phat_launch(const char* who, const R* X, double* psi, int* status, int B, int D, int F, int T, int f_lo, int f_hi,
                       void* stream) {
  ALVQ_REQUIRE(X && psi && status, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(phat_check_band(who, B, D, F, f_lo, f_hi));
  ALVQ_TRY(check_frames(who, T));
  const size_t row_bytes = 16 * (size_t)D * T;
  const bool row_lds = option(OPT_PHAT_LDS) != 0 && row_bytes <= (size_t)PHAT_LDS_LIMIT;
  static DeviceOnce attr;
  if (attr.need())
    (void)hipFuncSetAttribute((const void*)phat_kernel<R, true>, hipFuncAttributeMaxDynamicSharedMemorySize, PHAT_LDS_LIMIT);
  const PhatArgs args{X, (double2*)psi, B, D, F, T, f_lo, f_hi};
  const dim3 grid((unsigned)((long)B * F));
  if (row_lds)
    hipLaunchKernelGGL((phat_kernel<R, true>), grid, dim3(PHAT_THREADS), row_bytes, (hipStream_t)stream, args);
  else
    hipLaunchKernelGGL((phat_kernel<R, false>), grid, dim3(PHAT_THREADS), 0, (hipStream_t)stream, args);
  hipLaunchKernelGGL(phat_status_kernel, dim3(B), dim3(PHAT_THREADS), 0, (hipStream_t)stream, (const double2*)psi,
                     (const double*)nullptr, (const double*)nullptr, status, phat_pairs(D), F, f_lo, f_hi, D, 0, 0L, 0L);
  return check_launch(who);
}

extern "C" int alvq_phat_cross_spectra_f32(const float* X, double* psi, int* status, int B, int D, int F, int T, int f_lo,
                                           int f_hi, void* stream) {
  return phat_launch("alvq_phat_cross_spectra_f32", X, psi, status, B, D, F, T, f_lo, f_hi, stream);
}

extern "C" int alvq_phat_cross_spectra_f64(const double* X, double* psi, int* status, int B, int D, int F, int T, int f_lo,
                                           int f_hi, void* stream) {
  return phat_launch("alvq_phat_cross_spectra_f64", X, psi, status, B, D, F, T, f_lo, f_hi, stream);
}

extern "C" int alvq_gcc_phat_f64(const double* psi, double* r, int B, int D, int n_fft, int L, int f_lo, int f_hi, void* stream) {
  const char* who = "alvq_gcc_phat_f64";
  ALVQ_REQUIRE(psi && r, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(check_nfft(who, n_fft));
  const int F = n_fft / 2 + 1;
  ALVQ_TRY(phat_check_band(who, B, D, F, f_lo, f_hi));
  ALVQ_REQUIRE(L >= 0 && L <= n_fft / 2, ALVQ_EINVAL, "%s: L=%d (need 0 <= L <= n_fft / 2 = %d)", who, L, n_fft / 2);
  const long total = (long)B * phat_pairs(D) * (2L * L + 1);
  const long blocks = (total + PHAT_THREADS - 1) / PHAT_THREADS;
  ALVQ_REQUIRE(blocks <= INT_MAX, ALVQ_EINVAL, "%s: B P (2 L + 1) = %ld is too large", who, total);
  hipLaunchKernelGGL(gcc_kernel, dim3((unsigned)blocks), dim3(PHAT_THREADS), 0, (hipStream_t)stream, (const double2*)psi, r, total,
                     F, n_fft, L, f_lo, f_hi, phat_band_weight(n_fft, f_lo, f_hi));
  return check_launch(who);
}

template <int D>
static void srp_map_launch(const SrpArgs& args, bool psi_lds, size_t lds, dim3 grid, hipStream_t stream) {
  static DeviceOnce attr;
  if (attr.need())
    (void)hipFuncSetAttribute((const void*)srp_map_kernel<D, true>, hipFuncAttributeMaxDynamicSharedMemorySize, PHAT_LDS_LIMIT);
  if (psi_lds)
    hipLaunchKernelGGL((srp_map_kernel<D, true>), grid, dim3(SRP_THREADS), lds, stream, args);
  else
    hipLaunchKernelGGL((srp_map_kernel<D, false>), grid, dim3(SRP_THREADS), 0, stream, args);
}

extern "C" int alvq_srp_phat_f64(const double* psi, const double* mics, const double* cand, double* map, int* best, int* status,
                                 int B, int D, int G, int64_t mics_stride, int64_t cand_stride, double fs, int n_fft, double c,
                                 int f_lo, int f_hi, void* stream) {
  const char* who = "alvq_srp_phat_f64";
  ALVQ_REQUIRE(psi && mics && cand && map && best && status, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(check_nfft(who, n_fft));
  const int F = n_fft / 2 + 1;
  ALVQ_TRY(phat_check_band(who, B, D, F, f_lo, f_hi));
  ALVQ_TRY(check_candidates(who, B, G));
  ALVQ_TRY(check_rates(who, fs, c));
  ALVQ_REQUIRE((mics_stride == 0 || mics_stride >= 3L * D) && (cand_stride == 0 || cand_stride >= 3L * G), ALVQ_EINVAL,
               "%s: mics_stride=%ld cand_stride=%ld (need 0 or >= 3 D, 0 or >= 3 G)", who, (long)mics_stride, (long)cand_stride);
  const int P = phat_pairs(D), Fb = f_hi - f_lo + 1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(phat_status_kernel, dim3(B), dim3(PHAT_THREADS), 0, s, (const double2*)psi, mics, cand, status, P, F, f_lo,
                     f_hi, D, G, (long)mics_stride, (long)cand_stride);
  const size_t lds = 16 * (size_t)P * Fb;
  const bool psi_lds = option(OPT_PHAT_LDS) != 0 && lds <= (size_t)PHAT_LDS_LIMIT;
  const SrpArgs args{(const double2*)psi, mics, cand, map, status, B, G, F, n_fft, f_lo, f_hi, (long)mics_stride, (long)cand_stride,
                     fs / (double)n_fft, c, (double)P * phat_band_weight(n_fft, f_lo, f_hi)};
  const dim3 grid((unsigned)(((long)G + SRP_THREADS - 1) / SRP_THREADS), (unsigned)B);
#define SRP_CALL(N) srp_map_launch<N>(args, psi_lds, lds, grid, s)
  ALVQ_FOR_2_TO_8(D, SRP_CALL)
#undef SRP_CALL
  hipLaunchKernelGGL((map_peak_kernel<true, PHAT_THREADS>), dim3(B), dim3(PHAT_THREADS), 0, s, (const double*)map,
                     (const int*)status, best, G);
  return check_launch(who);
}
