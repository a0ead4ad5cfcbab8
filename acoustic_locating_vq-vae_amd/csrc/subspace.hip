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
// music_map_kernel<D>  srp_map_kernel's structure: a workgroup owns an item and a tile of 256 candidates, a thread a candidate,
//                      and walks the band.  The D phasors z_d = e^{j pi x}, x = (2 f fs / n_fft) tau_d, come from that kernel's
//                      rotation recurrence, re-anchored by sincospi every SUB_ANCHOR = 8 bins (the same K-term in the tests'
//                      bound); a_d = conj(z_d).  The bin's eigenvalues and its K signal eigenvectors are read at addresses that
//                      do not depend on the thread (scalar loads, one fetch a wave).  p_k = sum_d conj(e_k[d]) a_d with d
//                      rising from the first term, s = sum_k |p_k|^2 with k rising over the columns D - K .. D - 1, the bin adds
//                      1 - s / D; bins rising; the sum is divided by the number of counted bins.  A thread shares nothing with
//                      its neighbours: a candidate has the same bits alone or in any grid, an item alone or in any batch.
// music_argmin_kernel  srp_argmax_kernel with the comparison turned round: the lowest index of the minimum, on every run.
// What the launches cost: DESIGN.md.
#include <cfloat>
#include <climits>
#include <cmath>

#include "array_wave.h"
#include "herm_eig.h"

namespace alvq {

constexpr int SUB_THREADS = 256;
constexpr int SUB_WAVES = SUB_THREADS / kWave;
constexpr int SUB_ANCHOR = 8;          // bins between two sincospi anchors of the rotation recurrence (srp_phat's)
constexpr int SUB_MAX_NFFT = 1 << 24;

// status bits of alvq_music_f64 (alvq_srp_phat_f64's)
constexpr int MUSIC_BAD_SPECTRUM = 1;  // a non-finite eigenvector or eigenvalue inside the band
constexpr int MUSIC_SILENT = 2;        // no counted bin: every eigenvalue inside the band is 0
constexpr int MUSIC_BAD_GEOMETRY = 4;  // a non-finite microphone or candidate coordinate

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
  const double* m = mics + (long)b * mics_stride;
  for (int e = tid; e < 3 * D; e += SUB_THREADS)
    if (!is_finite(m[e])) seen |= 4;
  const double* q = cand + (long)b * cand_stride;
  for (long e = tid; e < 3L * G; e += SUB_THREADS)
    if (!is_finite(q[e])) seen |= 4;
  seen = block_sum<kSequential, false, OpOr>(seen, s_flag);
  if (tid == 0)
    status[b] = ((seen & 1) ? MUSIC_BAD_SPECTRUM : 0) | ((seen & 2) ? 0 : MUSIC_SILENT) | ((seen & 4) ? MUSIC_BAD_GEOMETRY : 0);
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
    if (g < a.G) out[g] = (st & (MUSIC_BAD_SPECTRUM | MUSIC_BAD_GEOMETRY)) ? __longlong_as_double(0x7ff8000000000000LL) : 1.0;
    return;
  }
  if (g >= a.G) return;

  const double* q = a.cand + (long)b * a.cand_stride + 3 * g;
  const double* m = a.mics + (long)b * a.mics_stride;
  const double qx = q[0], qy = q[1], qz = q[2];
  double tau[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double dx = qx - m[3 * d], dy = qy - m[3 * d + 1], dz = qz - m[3 * d + 2];
    tau[d] = sqrt(dx * dx + dy * dy + dz * dz) / a.c;
  }
  double wc[D], ws[D], zc[D], zs[D];                                     // the step e^{j pi (2 fs / n_fft) tau_d}; z_d of the bin
#pragma unroll
  for (int d = 0; d < D; ++d) sincospi(2.0 * a.fs_over_n * tau[d], &ws[d], &wc[d]);

  const int Fb = a.f_hi - a.f_lo + 1;
  double acc = 0.0;
  int counted = 0;
  for (int k = 0; k < Fb; ++k) {
    const int f = a.f_lo + k;
    if (k % SUB_ANCHOR == 0) {                                           // the same bins in every thread
      const double kf = (double)(2 * f) * a.fs_over_n;
#pragma unroll
      for (int d = 0; d < D; ++d) sincospi(kf * tau[d], &zs[d], &zc[d]);
    } else {
#pragma unroll
      for (int d = 0; d < D; ++d) {                                      // z_d <- z_d w_d
        const double cn = fma(zc[d], wc[d], -(zs[d] * ws[d]));
        const double sn = fma(zc[d], ws[d], zs[d] * wc[d]);
        zc[d] = cn;
        zs[d] = sn;
      }
    }
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
        const double tr = e.x * zc[d] - e.y * zs[d];
        const double ti = -(e.x * zs[d]) - e.y * zc[d];
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

__global__ __launch_bounds__(SUB_THREADS) void music_argmin_kernel(const double* map, const int* status, int* best, int G) {
  __shared__ double s_val[SUB_WAVES];
  __shared__ int s_idx[SUB_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  if (status[b]) {                                                       // the same in every thread
    if (tid == 0) best[b] = -1;
    return;
  }
  const double* row = map + (long)b * G;
  double bv = INFINITY;
  int bi = INT_MAX;
  for (int g = tid; g < G; g += SUB_THREADS) {                           // g rising: the first minimum of the thread's candidates
    const double v = row[g];
    if (v < bv) {
      bv = v;
      bi = g;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov < bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    s_val[wv] = bv;
    s_idx[wv] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SUB_WAVES; ++w)
      if (s_val[w] < bv || (s_val[w] == bv && s_idx[w] < bi)) {
        bv = s_val[w];
        bi = s_idx[w];
      }
    best[b] = bi == INT_MAX ? -1 : bi;
  }
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
  ALVQ_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && F <= SUB_MAX_NFFT && (long)B * F <= INT_MAX, ALVQ_EINVAL,
               "%s: B=%d F=%d (need 1 <= B <= 65535, 1 <= F <= 2^24, B F <= 2^31 - 1)", who, B, F);
  ALVQ_TRY(check_mics(who, D, 2));
  ALVQ_REQUIRE(K >= 1 && K <= D - 1, ALVQ_EINVAL, "%s: K=%d (need 1 <= K <= D - 1 = %d)", who, K, D - 1);
  ALVQ_REQUIRE(G >= 1 && (long)B * G <= INT_MAX, ALVQ_EINVAL, "%s: G=%d (need G >= 1, B G <= 2^31 - 1)", who, G);
  ALVQ_REQUIRE(n_fft >= 2 && n_fft <= SUB_MAX_NFFT, ALVQ_EINVAL, "%s: n_fft=%d (need 2 <= n_fft <= 2^24)", who, n_fft);
  ALVQ_REQUIRE(f_lo >= 0 && f_lo <= f_hi && f_hi < F, ALVQ_EINVAL, "%s: band %d..%d (need 0 <= f_lo <= f_hi < F = %d)", who, f_lo,
               f_hi, F);
  ALVQ_REQUIRE(std::isfinite(fs) && fs > 0.0 && std::isfinite(c) && c > 0.0, ALVQ_EINVAL, "%s: fs=%g c=%g must be finite and > 0",
               who, fs, c);
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
  hipLaunchKernelGGL(music_argmin_kernel, dim3(B), dim3(SUB_THREADS), 0, s, (const double*)null, (const int*)status, best, G);
  return check_launch(who);
}
