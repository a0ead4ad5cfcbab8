// Energy decay curves and room-acoustic parameters of impulse responses (Schroeder's backward integration with least-squares
// line fits to the decay curve, ISO 3382): reverberation times T30 / T20 / EDT, clarity C50 / C80, definition D50 and the
// direct-to-reverberant ratio, per response, in float64.  The definitions are the comment on alvq_room_acoustics_* in
// include/alvq.h; tests/helpers/room_acoustics_ref.py restates them in numpy.
//
// One workgroup of 256 threads per response, no atomics, no workspace.  Everything rests on one routine, suffix_scan: the
// tail energies S(t) = sum_{s >= t} h[s]^2 over tiles of 1024 samples taken from the last tile to the first.  In a tile a wave
// owns 256 consecutive samples.  It loads them coalesced (lane i: samples i, i + 64, i + 128, i + 192), turns them through its
// own LDS rows so that lane i holds the samples 4 i .. 4 i + 3, sums those serially from the back, and scans the 64 lane totals
// with cross-lane shuffles: 1.5 shuffle steps a sample instead of the 6 of a scan in the loaded order.  The four wave totals go
// through LDS and every thread adds them from the back onto the carry of the tiles behind.
// S(t) = ((carry + the waves behind) + the lanes behind) + the lane's own suffix: one order that depends on n alone, so a
// response has the same bits in any batch and on any run.  Nothing is reduced or compared across workgroups.
//   edc_kernel             scan once for S(0), scan again writing 10 (log10 S(t) - log10 S(0)) (a lane stores its four
//                          consecutive values).
//   room_acoustics_kernel  1. scan, each thread keeping its largest |h| (lowest index among equals; a NaN counts as the largest
//                             value) with S there; the workgroup's best is the onset n0 with S(n0), and S(0) says whether
//                             the row has energy;
//                          2. scan again with the fits: each thread adds the regression sums of its own samples for the three
//                             decay ranges (count, sum k, sum k^2, sum L, sum k L with k = t - n0: the k sums are exact
//                             integers up to n = 2^17) and keeps S at n0 + k50, n0 + k80, n0 - kdirect and n0 + kdirect + 1;
//                             the workgroup adds the threads' sums by butterfly and wave order, thread 0 closes the fits
//                             and the ratios.
//                          The level L(t) = 10 (log10 S(t) - log10 S(n0)), clamped at 0 (S(t) <= S(n0) but for rounding), is
//                          evaluated only where S(t) >= S(n0) * 2.5e-4 (-36 dB): below the lowest threshold nothing is fitted.
// Both passes are bound by float64 arithmetic, not by memory: the second read of a row comes from the L2.
#include <cfloat>
#include <climits>
#include <cmath>

#include "alvq_common.h"

namespace alvq {

constexpr int RA_THREADS = 256;
constexpr int RA_WAVES = RA_THREADS / kWave;
constexpr int RA_ITEMS = 4;                              // samples per thread and tile
constexpr int RA_WAVE_TILE = kWave * RA_ITEMS;           // consecutive samples per wave and tile
constexpr int RA_TILE = RA_THREADS * RA_ITEMS;
constexpr int RA_MAX_N = 1 << 24;

// status bits of alvq_room_acoustics_*
constexpr int RA_BAD_ENERGY = 1;       // S(0) is 0 or not finite: every output NaN
constexpr int RA_SHORT_RANGE = 2;      // a decay range held fewer than two samples: that output NaN
constexpr int RA_NO_LATE_ENERGY = 4;   // a late / reverberant energy was 0: that ratio +inf

// The LDS of one scan: each wave's 256 samples of the tile (to turn the coalesced order into four consecutive samples a lane)
// and the waves' totals, alternating between two buffers so that a tile needs one barrier.
struct RaScanLds {
  alignas(16) double xs[RA_WAVES][RA_WAVE_TILE];
  double wtot[2][RA_WAVES];
};

__device__ __forceinline__ void ra_wave_sync() {   // orders this wave's LDS writes and reads (its own rows of xs only)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Calls f(t, S(t), h(t)) for every t in [0, n), S(t) = sum_{s >= t} h(s)^2 with h(t) = ld(t), from the last tile to the first
// and, in a thread, in rising t within a tile.  The caller puts a __syncthreads() between two scans.
template <typename Ld, typename F>
__device__ __forceinline__ void suffix_scan(int n, Ld ld, RaScanLds& lds, F f) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* mine = lds.xs[wv];
  double carry = 0.0, nxt[RA_ITEMS];
  int base = (n - 1) / RA_TILE * RA_TILE;
  auto fetch = [&](int tile, double* dst) {        // lane i of wave w: samples w * 256 + i, + 64, + 128, + 192 of the tile
#pragma unroll
    for (int j = 0; j < RA_ITEMS; ++j) {
      const int t = tile + wv * RA_WAVE_TILE + j * kWave + lane;
      dst[j] = t < n ? ld(t) : 0.0;
    }
  };
  fetch(base, nxt);
  for (int p = 0; base >= 0; base -= RA_TILE, p ^= 1) {
    ra_wave_sync();                                // the tile before has been read out of xs
#pragma unroll
    for (int j = 0; j < RA_ITEMS; ++j) mine[j * kWave + lane] = nxt[j];
    if (base >= RA_TILE) fetch(base - RA_TILE, nxt);   // the next tile's samples are on their way during this tile's scan
    ra_wave_sync();
    double v[RA_ITEMS], s[RA_ITEMS];               // samples 4 i .. 4 i + 3 of the wave's 256, the suffix sums of their squares
#pragma unroll
    for (int i = 0; i < RA_ITEMS; ++i) {
      v[i] = mine[RA_ITEMS * lane + i];
      s[i] = v[i] * v[i];
    }
#pragma unroll
    for (int i = RA_ITEMS - 2; i >= 0; --i) s[i] += s[i + 1];
    double W = s[0];                               // suffix sums of the lanes' totals across the wave
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const double u = __shfl_down(W, o, kWave);
      if (lane + o < kWave) W += u;
    }
    double after = __shfl_down(W, 1, kWave);       // what the lanes behind this one hold
    if (lane == kWave - 1) after = 0.0;
    if (lane == 0) lds.wtot[p][wv] = W;
    __syncthreads();
    double run = carry, behind = 0.0;
#pragma unroll
    for (int w = RA_WAVES - 1; w >= 0; --w) {
      if (w == wv) behind = run;
      run += lds.wtot[p][w];
    }
    carry = run;
    behind += after;
    const int t0 = base + wv * RA_WAVE_TILE + RA_ITEMS * lane;
#pragma unroll
    for (int i = 0; i < RA_ITEMS; ++i)
      if (t0 + i < n) f(t0 + i, behind + s[i], v[i]);
  }
}

template <typename T>
__global__ __launch_bounds__(RA_THREADS) void edc_kernel(const T* __restrict__ h, double* __restrict__ edc_db, int n) {
  __shared__ RaScanLds lds;
  __shared__ double s_total;
  const T* x = h + (long)blockIdx.x * n;
  double* y = edc_db + (long)blockIdx.x * n;
  auto ld = [&](int t) { return (double)x[t]; };
  suffix_scan(n, ld, lds, [&](int t, double S, double) {
    if (t == 0) s_total = S;
  });
  __syncthreads();
  const double total = s_total;
  if (!(total > 0.0 && total <= DBL_MAX)) {
    for (int t = threadIdx.x; t < n; t += RA_THREADS) y[t] = NAN;
    return;
  }
  const double lg0 = log10(total);
  suffix_scan(n, ld, lds, [&](int t, double S, double) { y[t] = fmin(10.0 * (log10(S) - lg0), 0.0); });
}

struct RaFit {            // regression sums of one decay range over this thread's samples
  double m, sk, skk, sl, skl;
};

// -60 / slope (dB/s) of the least-squares line through the samples the sums hold; NaN and RA_SHORT_RANGE below two samples
__device__ __forceinline__ double ra_decay_time(const double* s, double fs, int& st) {
  if (s[0] < 2.0) {
    st |= RA_SHORT_RANGE;
    return NAN;
  }
  const double slope = (s[0] * s[4] - s[1] * s[3]) / (s[0] * s[2] - s[1] * s[1]);   // dB per sample
  return -60.0 / (slope * fs);
}

__device__ __forceinline__ double ra_ratio_db(double early, double late, int& st) {
  if (late == 0.0) {
    st |= RA_NO_LATE_ENERGY;
    return INFINITY;
  }
  return 10.0 * log10(early / late);
}

// |v| as an integer that orders like the magnitude, every NaN above infinity
__device__ __forceinline__ unsigned long long ra_mag_key(double v) {
  return v != v ? 0x7ff8000000000000ull : (unsigned long long)__double_as_longlong(fabs(v));
}

template <typename T>
__global__ __launch_bounds__(RA_THREADS) void room_acoustics_kernel(const T* __restrict__ h, double* __restrict__ out,
                                                                    int* __restrict__ onset, int* __restrict__ status, int n,
                                                                    double fs, int k50, int k80, int kdirect) {
  __shared__ RaScanLds lds;
  __shared__ double s_red[RA_WAVES][15];
  __shared__ double s_cap[5], s_S[RA_WAVES];
  __shared__ unsigned long long s_key[RA_WAVES];
  __shared__ int s_idx[RA_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  const T* x = h + (long)b * n;

  auto ld = [&](int t) { return (double)x[t]; };

  // 1. scan for the onset (largest key, lowest index among equals), its tail energy and the row's energy
  unsigned long long key = 0;
  int idx = INT_MAX;
  double S_at = 0.0;
  suffix_scan(n, ld, lds, [&](int t, double S, double v) {
    const unsigned long long k = ra_mag_key(v);
    if (k > key || (k == key && t < idx)) {
      key = k;
      idx = t;
      S_at = S;
    }
    if (t == 0) s_cap[0] = S;
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long k = __shfl_xor(key, o, kWave);
    const int i = __shfl_xor(idx, o, kWave);
    const double S = __shfl_xor(S_at, o, kWave);
    if (k > key || (k == key && i < idx)) {
      key = k;
      idx = i;
      S_at = S;
    }
  }
  if (lane == 0) {
    s_key[wv] = key;
    s_idx[wv] = idx;
    s_S[wv] = S_at;
  }
  if (tid >= 1 && tid < 5) s_cap[tid] = 0.0;     // S(n) = 0: a position clipped to n is never met by the scan
  __syncthreads();
  int best = 0;
#pragma unroll
  for (int w = 1; w < RA_WAVES; ++w)
    if (s_key[w] > s_key[best] || (s_key[w] == s_key[best] && s_idx[w] < s_idx[best])) best = w;
  const int n0 = s_idx[best];
  const double total = s_cap[0], S0 = s_S[best];
  if (!(total > 0.0 && total <= DBL_MAX)) {
    if (tid == 0) {
      for (int i = 0; i < 7; ++i) out[7 * (long)b + i] = NAN;
      onset[b] = n0;
      status[b] = RA_BAD_ENERGY;
    }
    return;
  }

  // 2. scan again with the fits, keeping the tail energies the ratios need
  const double hi[3] = {-5.0, -5.0, 0.0}, lo[3] = {-35.0, -25.0, -10.0};   // t30, t20, edt
  const double lg0 = log10(S0), floor_S = S0 * 2.5e-4;
  RaFit fit[3] = {};
  const long nl = n;
  const int at[4] = {(int)min((long)n0 + k50, nl), (int)min((long)n0 + k80, nl), (int)max((long)n0 - kdirect, 0L),
                     (int)min((long)n0 + kdirect + 1, nl)};
  suffix_scan(n, ld, lds, [&](int t, double S, double) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (t == at[i]) s_cap[1 + i] = S;
    if (t < n0 || !(S >= floor_S)) return;
    const double L = fmin(10.0 * (log10(S) - lg0), 0.0), k = (double)(t - n0);
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (L >= lo[r] && L <= hi[r]) {
        fit[r].m += 1.0;
        fit[r].sk += k;
        fit[r].skk += k * k;
        fit[r].sl += L;
        fit[r].skl += k * L;
      }
  });
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double s[5] = {wave_sum(fit[r].m), wave_sum(fit[r].sk), wave_sum(fit[r].skk), wave_sum(fit[r].sl), wave_sum(fit[r].skl)};
    if (lane == 0)
      for (int i = 0; i < 5; ++i) s_red[wv][5 * r + i] = s[i];
  }
  __syncthreads();
  if (tid != 0) return;
  double s[15];
  for (int i = 0; i < 15; ++i) s[i] = combine_waves<RA_WAVES, kSequential, 15>(&s_red[0][i]);
  int st = 0;
  double* o = out + 7 * (long)b;
  for (int r = 0; r < 3; ++r) o[r] = ra_decay_time(s + 5 * r, fs, st);
  o[3] = ra_ratio_db(S0 - s_cap[1], s_cap[1], st);
  o[4] = ra_ratio_db(S0 - s_cap[2], s_cap[2], st);
  o[5] = (S0 - s_cap[1]) / S0;
  o[6] = ra_ratio_db(s_cap[3] - s_cap[4], s_cap[4], st);
  onset[b] = n0;
  status[b] = st;
}

}  // namespace alvq

using namespace alvq;

static int ra_check_rows(const char* who, const void* h, const void* out, int B, int n) {
  ALVQ_REQUIRE(h && out, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(B >= 1 && n >= 2 && n <= RA_MAX_N, ALVQ_EINVAL, "%s: B=%d n=%d (need B >= 1, 2 <= n <= 2^24)", who, B, n);
  return ALVQ_OK;
}

template <typename T>
static int edc_launch(const char* who, const T* h, double* edc_db, int B, int n, void* stream) {
  const int rc = ra_check_rows(who, h, edc_db, B, n);
  if (rc != ALVQ_OK) return rc;
  hipLaunchKernelGGL(edc_kernel<T>, dim3(B), dim3(RA_THREADS), 0, (hipStream_t)stream, h, edc_db, n);
  return check_launch(who);
}

template <typename T>
static int room_acoustics_launch(const char* who, const T* h, double* out, int* onset, int* status, int B, int n, double fs,
                                 int k50, int k80, int kdirect, void* stream) {
  ALVQ_REQUIRE(onset && status, ALVQ_EINVAL, "%s: null pointer", who);
  const int rc = ra_check_rows(who, h, out, B, n);
  if (rc != ALVQ_OK) return rc;
  ALVQ_REQUIRE(std::isfinite(fs) && fs > 0.0, ALVQ_EINVAL, "%s: fs=%g must be > 0", who, fs);
  ALVQ_REQUIRE(k50 >= 0 && k80 >= 0 && kdirect >= 0, ALVQ_EINVAL, "%s: k50=%d k80=%d kdirect=%d (need >= 0)", who, k50, k80,
               kdirect);
  hipLaunchKernelGGL(room_acoustics_kernel<T>, dim3(B), dim3(RA_THREADS), 0, (hipStream_t)stream, h, out, onset, status,
                     n, fs, k50, k80, kdirect);
  return check_launch(who);
}

extern "C" int alvq_edc_f32(const float* h, double* edc_db, int B, int n, void* stream) {
  return edc_launch("alvq_edc_f32", h, edc_db, B, n, stream);
}

extern "C" int alvq_edc_f64(const double* h, double* edc_db, int B, int n, void* stream) {
  return edc_launch("alvq_edc_f64", h, edc_db, B, n, stream);
}

extern "C" int alvq_room_acoustics_f32(const float* h, double* out, int* onset, int* status, int B, int n, double fs, int k50,
                                       int k80, int kdirect, void* stream) {
  return room_acoustics_launch("alvq_room_acoustics_f32", h, out, onset, status, B, n, fs, k50, k80, kdirect, stream);
}

extern "C" int alvq_room_acoustics_f64(const double* h, double* out, int* onset, int* status, int B, int n, double fs, int k50,
                                       int k80, int kdirect, void* stream) {
  return room_acoustics_launch("alvq_room_acoustics_f64", h, out, onset, status, B, n, fs, k50, k80, kdirect, stream);
}
