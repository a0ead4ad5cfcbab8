// The one owner of what the maps over candidate source positions share (included by srp_phat.hip, subspace.hip and, for the
// delay, the geometry bit and the host rules, beamform.hip):
//   steering walk  steer_delay, tau_d = |q - m_d| / c, and SteerWalk<D>: a candidate's D delays, the step phasors
//                  w_d = e^{j pi (2 fs / n_fft) tau_d} and the phasors z_d = e^{j pi x}, x = (2 f fs / n_fft) tau_d, of the current
//                  bin.  Along f the phasors follow a rotation recurrence, re-anchored every kSteerAnchor = 8 bins: at the bins
//                  f_lo, f_lo + 8, ... they come from sincospi on x itself, at the 7 bins between from z_d <- z_d w_d, four
//                  fused multiply-adds in place of a sincospi, which halved the SRP launch.  A step leaves a
//                  relative error of at most 3 u on a phasor, so at most 21 u before the next anchor: the K-term of both
//                  families' bounds (tests/helpers/srp_ref.py::ANCHOR).  The library is built with -ffp-contract=off, so the
//                  bits follow the text here as they did in the kernels.
//   peak kernel    map_peak_kernel<MAXIMUM, THREADS>, one workgroup an item: a thread keeps the first extremum of its candidates
//                  g = tid, tid + THREADS, ...; then (value, index) pairs meet in a butterfly and over the waves under "better
//                  value, or equal value and lower index", which is associative and commutative: the lowest index of the
//                  extremum, on every run; -1 for an item with a status, or when no candidate compares (an all-NaN row).
//   status         the three bits of a map's status word, the strided scan of an item's coordinates, and the status word from
//                  what a status kernel has seen.
//   host rules     n_fft, the band, the candidate count, fs and c: each with the one message text the callers and tests see.
// What is not here, on purpose: the accumulation over pairs (SRP) and over signal eigenvectors (MUSIC), which stay in their
// kernels; the spectrum parts of the two status kernels (psi pairs against eigenvectors and eigenvalues); bf_steer_kernel's
// phasor, a sincospi of tau_d - tau_ref at every bin, which is a different formula; alvq_music_f64's B, F rule, which carries
// F <= 2^24 inside its message.  And the fill of a map tile whose item has a status (NaN for the bits 1 and 4, else the
// family's idle value) stays one line at the top of each map kernel: as a helper here, storing or only returning the value,
// it cost every music_map_kernel<D> and every srp_map_kernel<D, false> the scalar loads of its uniform addresses
// (music_map_kernel<5>: 68 -> 98 VGPRs, 7 -> 4 waves a SIMD; srp_map_kernel<8, false>: 94 -> 112, 5 -> 4).
// The measurements: profiles/steered_map_ab.txt.
#pragma once
#include "array_wave.h"

namespace alvq {

constexpr int kSteerAnchor = 8;        // bins between two sincospi anchors of the rotation recurrence
constexpr int kMaxNfft = 1 << 24;

// status bits of alvq_phat_cross_spectra_*, alvq_srp_phat_f64 and alvq_music_f64; alvq_steering_vectors_f64 sets the last
constexpr int MAP_BAD_SPECTRUM = 1;    // a non-finite psi, eigenvector or eigenvalue inside the band
constexpr int MAP_SILENT = 2;          // every psi, or every eigenvalue, inside the band is 0
constexpr int MAP_BAD_GEOMETRY = 4;    // a non-finite microphone, candidate or source coordinate

// ---------------------------------------------------------------------------------------------------------------- steering walk
__device__ __forceinline__ double steer_delay(double qx, double qy, double qz, const double* m, int d, double c) {
  const double dx = qx - m[3 * d], dy = qy - m[3 * d + 1], dz = qz - m[3 * d + 2];
  return sqrt(dx * dx + dy * dy + dz * dz) / c;
}

template <int D>
struct SteerWalk {
  double tau[D], wc[D], ws[D], zc[D], zs[D];                             // the delays; the step; z_d of the bin

  __device__ __forceinline__ SteerWalk(const double* m, const double* q, double c, double fs_over_n) {
    const double qx = q[0], qy = q[1], qz = q[2];
#pragma unroll
    for (int d = 0; d < D; ++d) tau[d] = steer_delay(qx, qy, qz, m, d, c);
#pragma unroll
    for (int d = 0; d < D; ++d) sincospi(2.0 * fs_over_n * tau[d], &ws[d], &wc[d]);
  }

  // to bin f = f_lo + k; k rises by one from 0
  __device__ __forceinline__ void move(int k, int f, double fs_over_n) {
    if (k % kSteerAnchor == 0) {                                         // the same bins in every thread
      const double kf = (double)(2 * f) * fs_over_n;
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
  }
};

// ------------------------------------------------------------------------------------------------------------------ peak kernel
template <bool MAXIMUM>
__device__ __forceinline__ bool peak_better(double v, double than) { return MAXIMUM ? v > than : v < than; }

template <bool MAXIMUM, int THREADS>
__global__ __launch_bounds__(THREADS) void map_peak_kernel(const double* map, const int* status, int* best, int G) {
  constexpr int WAVES = THREADS / kWave;
  __shared__ double s_val[WAVES];
  __shared__ int s_idx[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  if (status[b]) {                                                       // the same in every thread
    if (tid == 0) best[b] = -1;
    return;
  }
  const double* row = map + (long)b * G;
  double bv = MAXIMUM ? -INFINITY : INFINITY;
  int bi = INT_MAX;
  for (int g = tid; g < G; g += THREADS) {                               // g rising: the first extremum of the thread's candidates
    const double v = row[g];
    if (peak_better<MAXIMUM>(v, bv)) {
      bv = v;
      bi = g;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (peak_better<MAXIMUM>(ov, bv) || (ov == bv && oi < bi)) {
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
    for (int w = 1; w < WAVES; ++w)
      if (peak_better<MAXIMUM>(s_val[w], bv) || (s_val[w] == bv && s_idx[w] < bi)) {
        bv = s_val[w];
        bi = s_idx[w];
      }
    best[b] = bi == INT_MAX ? -1 : bi;
  }
}

// ----------------------------------------------------------------------------------------------------------------------- status
// What a status kernel has seen: 1 a non-finite spectrum value, 2 a non-zero one, 4 a non-finite coordinate.  The geometry
// part, over an item's 3 D microphone and 3 G candidate coordinates, a thread every THREADS-th of them:
template <int THREADS>
__device__ __forceinline__ int geometry_seen(const double* m, const double* q, int D, int G, int tid) {
  int seen = 0;
  for (int e = tid; e < 3 * D; e += THREADS)
    if (!is_finite(m[e])) seen |= 4;
  for (long e = tid; e < 3L * G; e += THREADS)
    if (!is_finite(q[e])) seen |= 4;
  return seen;
}
__device__ __forceinline__ int map_status(int seen) {
  return ((seen & 1) ? MAP_BAD_SPECTRUM : 0) | ((seen & 2) ? 0 : MAP_SILENT) | ((seen & 4) ? MAP_BAD_GEOMETRY : 0);
}

// ------------------------------------------------------------------------------------------------------------------- host rules
inline int check_nfft(const char* who, int n_fft) {
  ALVQ_REQUIRE(n_fft >= 2 && n_fft <= kMaxNfft, ALVQ_EINVAL, "%s: n_fft=%d (need 2 <= n_fft <= 2^24)", who, n_fft);
  return ALVQ_OK;
}
// alvq_steering_vectors_f64 is given F by its caller and bounds it in the same rule
inline int check_nfft(const char* who, int n_fft, int F) {
  ALVQ_REQUIRE(n_fft >= 2 && n_fft <= kMaxNfft && F <= kMaxNfft, ALVQ_EINVAL, "%s: n_fft=%d F=%d (need 2 <= n_fft <= 2^24, F <= 2^24)",
               who, n_fft, F);
  return ALVQ_OK;
}
inline int check_band(const char* who, int f_lo, int f_hi, int F) {
  ALVQ_REQUIRE(f_lo >= 0 && f_lo <= f_hi && f_hi < F, ALVQ_EINVAL, "%s: band %d..%d (need 0 <= f_lo <= f_hi < F = %d)", who, f_lo,
               f_hi, F);
  return ALVQ_OK;
}
inline int check_candidates(const char* who, int B, int G) {
  ALVQ_REQUIRE(G >= 1 && (long)B * G <= INT_MAX, ALVQ_EINVAL, "%s: G=%d (need G >= 1, B G <= 2^31 - 1)", who, G);
  return ALVQ_OK;
}
inline int check_rates(const char* who, double fs, double c) {
  ALVQ_REQUIRE(std::isfinite(fs) && fs > 0.0 && std::isfinite(c) && c > 0.0, ALVQ_EINVAL, "%s: fs=%g c=%g must be finite and > 0",
               who, fs, c);
  return ALVQ_OK;
}

}  // namespace alvq
