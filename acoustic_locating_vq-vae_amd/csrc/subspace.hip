// Subspace methods on a microphone array's spatial covariances: the batched Hermitian eigendecomposition (order 1 .. 8, one
// problem per item and frequency bin) and the MUSIC null spectrum over candidate positions with its arg-min (Schmidt 1986).
// The definitions are the comment on alvq_eigh_f64 / alvq_music_f64 in include/alvq.h; tests/helpers/subspace_ref.py restates
// them in numpy.  All arithmetic is float64.
//
// sub_eigh_kernel      a wave a matrix, four matrices a workgroup, no LDS and no barrier: csrc/herm_eig.h does the work.  The
//                      lane 8 r + c reads entry (max(r, c), min(r, c)) itself (the upper triangle as the conjugate of the
//                      lower, the diagonal's real part alone) and stores entry (r, rank(c)) of V: columns land in ascending
//                      order of their eigenvalues.  The grid is capped at kMaxBlocks workgroups; a wave strides over the
//                      matrices beyond, whole.
// music_status_kernel  one workgroup an item: the OR over the item's band of V and lambda (a non-finite value; a non-zero
//                      eigenvalue) and over its coordinates.  No atomics: wave_or, then the waves through LDS.
// music_map_kernel<D>  a workgroup owns an item and a tile of 256 candidates, a thread a candidate, and walks the band.  The D
//                      phasors z_d = e^{j pi x}, x = (2 f fs / n_fft) tau_d, come from csrc/steered_map.h's SteerWalk<D>: a
//                      rotation recurrence, re-anchored by sincospi every 8 bins (the K-term in the tests' bound);
//                      a_d = conj(z_d).  The bin's eigenvalues and its K signal eigenvectors are read at addresses that
//                      do not depend on the thread (scalar loads, one fetch a wave).  p_k = sum_d conj(e_k[d]) a_d with d
//                      rising from the first term, s = sum_k |p_k|^2 with k rising over the columns D - K .. D - 1, the bin adds
//                      1 - s / D; bins rising; the sum is divided by the number of counted bins.  A thread shares nothing with
//                      its neighbours: a candidate has the same bits alone or in any grid, an item alone or in any batch.
// The arg-min is csrc/steered_map.h's map_peak_kernel<false, 256>; the status bits, the coordinate scan and the host rules of
// n_fft, the band, G, fs and c are that header's too.
// What the launches cost: DESIGN.md.
#include "herm_eig.h"
#include "steered_map.h"

namespace alvq {

constexpr int SUB_THREADS = 256;
constexpr int SUB_WAVES = SUB_THREADS / kWave;

// --------------------------------------------------------------------------------------------------------- eigendecomposition
__global__ __launch_bounds__(SUB_THREADS) void sub_eigh_kernel(const double2* A, double* lam, double2* V, int* status, long n, int D) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane >> 3, c = lane & 7;
  const bool in = r < D && c < D;
  // the grid is capped: a wave strides over its matrices, whole, and meets no barrier anywhere
  for (long i = (long)blockIdx.x * SUB_WAVES + wv; i < n; i += (long)gridDim.x * SUB_WAVES) {
    const double2* Ag = A + i * (D * D);
    double2 a = make_double2(0.0, 0.0);
    if (in) {
      if (r > c) {
        a = Ag[r * D + c];
      } else if (r == c) {
        a = make_double2(Ag[r * D + c].x, 0.0);
      } else {
        const double2 t = Ag[c * D + r];
        a = make_double2(t.x, -t.y);
      }
    }
    double2 v;
    const HermEig e = herm_eig(a, v, D, lane);
    if (in) V[i * (D * D) + r * D + e.rank] = v;
    if (r == 0 && c < D) lam[i * D + e.rank] = e.lam;
    if (lane == 0) status[i] = e.status;
  }
}

// ---------------------------------------------------------------------------------------------------------------------- MUSIC
__global__ __launch_bounds__(SUB_THREADS) void music_status_kernel(const double2* V, const double* lam, const double* mics,
                                                                    const double* cand, int* status, int D, int F, int G, int f_lo,
                                                                    int f_hi, long mics_stride, long cand_stride) {
  __shared__ int s_flag[SUB_WAVES];
  const int tid = threadIdx.x, b = blockIdx.x;
  int seen = 0;                                                          // 1 non-finite, 2 a non-zero eigenvalue, 4 bad coordinate
  const long nb = (long)(f_hi - f_lo + 1);
  const double2* Vg = V + ((long)b * F + f_lo) * (D * D);
  for (long e = tid; e < nb * D * D; e += SUB_THREADS) {
    const double2 x = Vg[e];
    if (!is_finite(x.x) || !is_finite(x.y)) seen |= 1;
  }
  const double* lg = lam + ((long)b * F + f_lo) * D;
  for (long e = tid; e < nb * D; e += SUB_THREADS) {
    const double x = lg[e];
    if (!is_finite(x)) seen |= 1;
    if (x != 0.0) seen |= 2;
  }
  seen |= geometry_seen<SUB_THREADS>(mics + (long)b * mics_stride, cand + (long)b * cand_stride, D, G, tid);
  seen = block_sum<kSequential, false, OpOr>(seen, s_flag);
  if (tid == 0) status[b] = map_status(seen);
}

struct MusicArgs {
  const double2* V;
  const double* lam;
  const double* mics;
  const double* cand;
  double* null;
  const int* status;
  int G, F, K, f_lo, f_hi;
  long mics_stride, cand_stride;
  double fs_over_n, c;
};

template <int D>
__global__ __launch_bounds__(SUB_THREADS) void music_map_kernel(MusicArgs a) {
  const int tid = threadIdx.x, b = blockIdx.y;
  const long g = (long)blockIdx.x * SUB_THREADS + tid;
  double* out = a.null + (long)b * a.G;
  const int st = a.status[b];                                            // the same in every thread of the workgroup
  if (st) {
    if (g < a.G) out[g] = (st & (MAP_BAD_SPECTRUM | MAP_BAD_GEOMETRY)) ? __longlong_as_double(0x7ff8000000000000LL) : 1.0;
    return;
  }
  if (g >= a.G) return;

  SteerWalk<D> z(a.mics + (long)b * a.mics_stride, a.cand + (long)b * a.cand_stride + 3 * g, a.c, a.fs_over_n);
  const int Fb = a.f_hi - a.f_lo + 1;
  double acc = 0.0;
  int counted = 0;
  for (int k = 0; k < Fb; ++k) {
    const int f = a.f_lo + k;
    z.move(k, f, a.fs_over_n);
    const long bin = (long)b * a.F + f;                                  // uniform addresses from here on
    const double* lg = a.lam + bin * D;
    bool live = false;
#pragma unroll
    for (int d = 0; d < D; ++d) live = live || lg[d] != 0.0;
    if (!live) continue;                                                 // a silent bin is not counted
    const double2* Vg = a.V + bin * (D * D);
    double s = 0.0;
    for (int col = D - a.K; col < D; ++col) {
      double pr = 0.0, pi = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {                                      // conj(e_d) a_d, a_d = zc - j zs
        const double2 e = Vg[d * D + col];
        const double tr = e.x * z.zc[d] - e.y * z.zs[d];
        const double ti = -(e.x * z.zs[d]) - e.y * z.zc[d];
        pr = d == 0 ? tr : pr + tr;
        pi = d == 0 ? ti : pi + ti;
      }
      s += pr * pr + pi * pi;
    }
    acc += 1.0 - s / (double)D;
    ++counted;
  }
  out[g] = acc / (double)counted;
}

}  // namespace alvq

using namespace alvq;

extern "C" int alvq_eigh_f64(const double* A, double* lam, double* V, int* status, int64_t n_matrices, int D, void* stream) {
  const char* who = "alvq_eigh_f64";
  ALVQ_REQUIRE(A && lam && V && status, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(n_matrices >= 1 && n_matrices <= INT_MAX, ALVQ_EINVAL, "%s: n_matrices=%ld (need 1 <= n_matrices <= 2^31 - 1)", who,
               (long)n_matrices);
  ALVQ_TRY(check_mics(who, D));
  hipLaunchKernelGGL(sub_eigh_kernel, capped_grid(((long)n_matrices + SUB_WAVES - 1) / SUB_WAVES), dim3(SUB_THREADS), 0,
                     (hipStream_t)stream, (const double2*)A, lam, (double2*)V, status, (long)n_matrices, D);
  return check_launch(who);
}

extern "C" int alvq_music_f64(const double* V, const double* lam, const double* mics, const double* cand, double* null, int* best,
                              int* status, int B, int D, int F, int G, int K, double fs, int n_fft, double c, int f_lo, int f_hi,
                              int mics_batched, int cand_batched, void* stream) {
  const char* who = "alvq_music_f64";
  ALVQ_REQUIRE(V && lam && mics && cand && null && best && status, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && F <= kMaxNfft && (long)B * F <= INT_MAX, ALVQ_EINVAL,
               "%s: B=%d F=%d (need 1 <= B <= 65535, 1 <= F <= 2^24, B F <= 2^31 - 1)", who, B, F);
  ALVQ_TRY(check_mics(who, D, 2));
  ALVQ_REQUIRE(K >= 1 && K <= D - 1, ALVQ_EINVAL, "%s: K=%d (need 1 <= K <= D - 1 = %d)", who, K, D - 1);
  ALVQ_TRY(check_candidates(who, B, G));
  ALVQ_TRY(check_nfft(who, n_fft));
  ALVQ_TRY(check_band(who, f_lo, f_hi, F));
  ALVQ_TRY(check_rates(who, fs, c));
  const long mics_stride = mics_batched ? 3L * D : 0L, cand_stride = cand_batched ? 3L * G : 0L;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(music_status_kernel, dim3(B), dim3(SUB_THREADS), 0, s, (const double2*)V, lam, mics, cand, status, D, F, G, f_lo,
                     f_hi, mics_stride, cand_stride);
  const MusicArgs args{(const double2*)V, lam, mics, cand, null, status, G, F, K, f_lo, f_hi, mics_stride, cand_stride,
                       fs / (double)n_fft, c};
  const dim3 grid((unsigned)(((long)G + SUB_THREADS - 1) / SUB_THREADS), (unsigned)B);
#define SUB_CALL(N) hipLaunchKernelGGL(music_map_kernel<N>, grid, dim3(SUB_THREADS), 0, s, args)
  ALVQ_FOR_2_TO_8(D, SUB_CALL)
#undef SUB_CALL
  hipLaunchKernelGGL((map_peak_kernel<false, SUB_THREADS>), dim3(B), dim3(SUB_THREADS), 0, s, (const double*)null,
                     (const int*)status, best, G);
  return check_launch(who);
}
