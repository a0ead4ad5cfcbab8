// What a listener gets from a waveform or a spectrogram, measured on the device in float64: rational resampling
// (scipy.signal.resample_poly's polyphase FIR), short-time objective intelligibility (STOI: Taal, Hendriks, Heusdens, Jensen
// 2011), scale-invariant SDR and the log-spectral distance of power spectrograms.  The definitions are the comments on
// alvq_resample_poly_*, alvq_stoi_f64, alvq_si_sdr_* and alvq_lsd_* in include/alvq.h; tests/helpers/speech_metrics_ref.py
// restates them in numpy.
//
// No atomics and nothing compared across workgroups: every sum runs in one order that depends on the row's own sizes alone, so
// a row has the same bits in any batch and on any run.  Every launch writes per-row results and status words that only later
// launches read: no host sync.
//   resample_poly_kernel   one thread per (row, output sample): the taps h[m down - j up + half] in rising j.  A filter of up
//                          to 4096 taps (every ratio to 10 or 16 kHz but those from 44.1 / 22.05 / 11.025 kHz) is copied to
//                          LDS by each workgroup and gathered there; a longer one is gathered from global memory.
//   STOI, four launches over a caller-owned workspace (frame energies, kept-frame lists, band envelopes):
//   stoi_energy_kernel     a wave per frame of the clean row: the energy of the windowed frame.
//   stoi_mask_kernel       a workgroup per row: the largest frame level, the frames within 40 dB of it, and their indices in
//                          order (ballot prefix sums over tiles of 256 frames): rows of one batch keep different numbers.
//   stoi_envelope_kernel   a workgroup per (row, kept frame m): frame m of the signal rebuilt by overlap-add is gathered from
//                          the kept frames m - 1, m, m + 1 (the rebuilt signal is never stored), windowed again, and a thread per
//                          bin takes the 512-point DFT directly from an LDS twiddle table for the bins the bands cover (7..218),
//                          clean and degraded together; 30 threads sum the band energies.
//   stoi_correlate_kernel  a workgroup per row: a thread per (band, segment of 30 frames) clips, centres, normalises and
//                          correlates; the workgroup's sum over 15 (M - 29) pairs is the value.
//   The framing here lies wholly inside the signal with a symmetric Hann window and a zero-padded 512-point DFT; the shared
//   framed DFT of dft_frames.h is centred, reflect-padded and periodic-windowed, so it is not used.
//   si_sdr_kernel          a workgroup per row, three passes (means, projection, energies): the later reads come from the L2.
//   lsd_kernel             a workgroup per spectrogram, a thread per frame column (coalesced across the workgroup).
#include <cfloat>
#include <climits>
#include <cmath>

#include "alvq_common.h"

namespace alvq {

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / kWave;
constexpr int SM_MAX_N = 1 << 24;
constexpr int SM_MAX_ROWS = 65535;        // rows ride on gridDim.y
constexpr int SM_MAX_RATE = 512;          // max(up, down) of the resampler

constexpr int ST_FRAME = 256, ST_HOP = 128, ST_NFFT = 512, ST_BANDS = 15, ST_SEG = 30;
constexpr double ST_EPS = 2.220446049250313e-16;   // 2^-52
constexpr double ST_RANGE_DB = 40.0;
constexpr double ST_CLIP = 6.623413251903491;    // 1 + 10^(15 / 20): beta = -15 dB
constexpr int ST_BAD_ENERGY = 1;          // fewer than 256 samples, or a clean row of zero or non-finite energy
constexpr int ST_FEW_FRAMES = 2;          // fewer than 30 frames kept

// ---------------------------------------------------------------------------------------------------------------- resampling
constexpr int RS_LDS_TAPS = 4096;         // a filter of up to this many taps (R <= 204) is staged in LDS

// STAGED: the workgroup copies the filter to LDS first and gathers its taps there; otherwise from global memory.  The
// arithmetic and its order are the same.
template <typename T, bool STAGED>
__global__ __launch_bounds__(SM_THREADS) void resample_poly_kernel(const T* __restrict__ x, const double* __restrict__ h,
                                                                   double* __restrict__ y, int n, long n_out, int up, int down,
                                                                   int half) {
  __shared__ double s_h[STAGED ? RS_LDS_TAPS : 1];
  if (STAGED) {
    for (int k = threadIdx.x; k <= 2 * half; k += SM_THREADS) s_h[k] = h[k];
    __syncthreads();
  }
  const long m = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (m >= n_out) return;
  const T* xr = x + (long)blockIdx.y * n;
  const long c = m * down + half;                       // tap index k = c - j up, 0 <= k <= 2 half
  const long lowest = c - 2L * half;
  const long j0 = lowest > 0 ? (lowest + up - 1) / up : 0;
  const long j1 = min(c / up, (long)n - 1);
  double acc = 0.0;
  for (long j = j0; j <= j1; ++j) acc += (double)xr[j] * (STAGED ? s_h[c - j * up] : h[c - j * up]);
  y[(long)blockIdx.y * n_out + m] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------- STOI
struct StoiBands {
  int lo[ST_BANDS], hi[ST_BANDS];
  int first, count;                       // the bins the DFT evaluates: first <= k < first + count <= 257, count <= 256
};

// the 258-point symmetric Hann window without its zero end points
__device__ __forceinline__ double stoi_window(int i) { return 0.5 - 0.5 * cospi(2.0 * (double)(i + 1) / (double)(ST_FRAME + 1)); }

__device__ __forceinline__ double stoi_level_db(double energy) { return 20.0 * log10(sqrt(energy) + ST_EPS); }

__global__ __launch_bounds__(SM_THREADS) void stoi_energy_kernel(const double* __restrict__ clean, double* __restrict__ energy,
                                                                 int n, int nf) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * SM_WAVES + (threadIdx.x >> 6);
  if (t >= nf) return;
  const double* x = clean + (long)blockIdx.y * n + (long)ST_HOP * t;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < ST_FRAME / kWave; ++q) {
    const int i = q * kWave + lane;
    const double v = stoi_window(i) * x[i];
    s += v * v;
  }
  s = wave_sum(s);
  if (lane == 0) energy[(long)blockIdx.y * nf + t] = s;
}

__global__ __launch_bounds__(SM_THREADS) void stoi_mask_kernel(const double* __restrict__ energy, int* __restrict__ kept,
                                                               int* __restrict__ kept_frames, int* __restrict__ status, int nf) {
  __shared__ double s_max[SM_WAVES];
  __shared__ int s_flag[SM_WAVES], s_cnt[2][SM_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  const double* e_row = energy + (long)b * nf;
  int* k_row = kept + (long)b * nf;

  // the largest frame level; whether any energy is not finite (flag bit 1) or positive (flag bit 2)
  double top = -INFINITY;
  int flag = 0;
  for (int t = tid; t < nf; t += SM_THREADS) {
    const double s = e_row[t];
    if (!(s >= 0.0 && s <= DBL_MAX)) flag |= 1;
    else {
      if (s > 0.0) flag |= 2;
      top = fmax(top, stoi_level_db(s));
    }
  }
  block_max_or<false>(top, flag, s_max, s_flag);
  if (flag != 2) {                         // no frame at all, an energy that is not finite, or no energy
    if (tid == 0) {
      kept_frames[b] = 0;
      status[b] = ST_BAD_ENERGY;
    }
    return;
  }

  // the kept frames' indices in order
  const double threshold = top - ST_RANGE_DB;
  int carry = 0;
  for (int base = 0, p = 0; base < nf; base += SM_THREADS, p ^= 1) {
    const int t = base + tid;
    const bool keep = t < nf && stoi_level_db(e_row[t]) > threshold;
    const unsigned long long votes = __ballot(keep);
    const int before = __popcll(votes & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[p][wv] = __popcll(votes);
    __syncthreads();                       // s_cnt alternates between two buffers: one barrier a tile
    int ahead = carry, all = carry;
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w) {
      if (w < wv) ahead += s_cnt[p][w];
      all += s_cnt[p][w];
    }
    if (keep) k_row[ahead + before] = t;   // ahead + before < number of kept frames <= nf
    carry = all;
  }
  if (tid == 0) {
    kept_frames[b] = carry;
    status[b] = carry < ST_SEG ? ST_FEW_FRAMES : 0;
  }
}

__global__ __launch_bounds__(SM_THREADS) void stoi_envelope_kernel(const double* __restrict__ clean,
                                                                   const double* __restrict__ degraded,
                                                                   const int* __restrict__ kept,
                                                                   const int* __restrict__ kept_frames, double* __restrict__ env,
                                                                   StoiBands bands, int n, int nf) {
  __shared__ double s_x[ST_FRAME], s_y[ST_FRAME], s_px[SM_THREADS], s_py[SM_THREADS];
  __shared__ double2 s_tw[ST_NFFT];
  const int tid = threadIdx.x, m = blockIdx.x, b = blockIdx.y;
  const int M = kept_frames[b];
  if (m >= M) return;
  const int* k_row = kept + (long)b * nf;
  const double* x = clean + (long)b * n;
  const double* y = degraded + (long)b * n;

  for (int j = tid; j < ST_NFFT; j += SM_THREADS) {
    double sn, cs;
    sincospi((double)j / (double)(ST_NFFT / 2), &sn, &cs);
    s_tw[j] = make_double2(cs, sn);
  }
  {
    // sample tid of frame m of the rebuilt signal: the kept frame m's own windowed sample plus that of the one neighbour
    // that overlaps it (m - 1 for the first half, m + 1 for the second), then the window again
    const int i = tid;
    const double w = stoi_window(i);
    const long at = (long)ST_HOP * k_row[m] + i;
    double vx = w * x[at], vy = w * y[at];
    const int other = i < ST_HOP ? m - 1 : m + 1;
    if (other >= 0 && other < M) {
      const int io = i < ST_HOP ? i + ST_HOP : i - ST_HOP;
      const double wo = stoi_window(io);
      const long ato = (long)ST_HOP * k_row[other] + io;
      vx += wo * x[ato];
      vy += wo * y[ato];
    }
    s_x[i] = w * vx;
    s_y[i] = w * vy;
  }
  __syncthreads();
  double px = 0.0, py = 0.0;
  if (tid < bands.count) {
    const int k = bands.first + tid;
    double xr = 0.0, xi = 0.0, yr = 0.0, yi = 0.0;
    for (int i = 0; i < ST_FRAME; ++i) {
      const double2 tw = s_tw[(k * i) & (ST_NFFT - 1)];
      const double a = s_x[i], c = s_y[i];
      xr += a * tw.x;
      xi -= a * tw.y;
      yr += c * tw.x;
      yi -= c * tw.y;
    }
    px = xr * xr + xi * xi;
    py = yr * yr + yi * yi;
  }
  s_px[tid] = px;
  s_py[tid] = py;
  __syncthreads();
  if (tid < 2 * ST_BANDS) {
    const int sig = tid / ST_BANDS, j = tid % ST_BANDS;
    const double* pw = sig ? s_py : s_px;
    double s = 0.0;
    for (int k = bands.lo[j]; k < bands.hi[j]; ++k) s += pw[k - bands.first];
    env[(((long)b * 2 + sig) * ST_BANDS + j) * nf + m] = sqrt(s);
  }
}

__global__ __launch_bounds__(SM_THREADS) void stoi_correlate_kernel(const double* __restrict__ env,
                                                                    const int* __restrict__ kept_frames,
                                                                    const int* __restrict__ status, double* __restrict__ value,
                                                                    int nf) {
  __shared__ double s_red[1][SM_WAVES];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (status[b] != 0) {
    if (tid == 0) value[b] = NAN;
    return;
  }
  const int segments = kept_frames[b] - ST_SEG + 1, pairs = ST_BANDS * segments;
  double acc[1] = {0.0};
  for (int p = tid; p < pairs; p += SM_THREADS) {
    const int j = p / segments, s0 = p % segments;
    const double* xe = env + (((long)b * 2 + 0) * ST_BANDS + j) * nf + s0;
    const double* ye = env + (((long)b * 2 + 1) * ST_BANDS + j) * nf + s0;
    double xs[ST_SEG], ys[ST_SEG];
    double xx = 0.0, yy = 0.0;
#pragma unroll
    for (int i = 0; i < ST_SEG; ++i) {
      xs[i] = xe[i];
      ys[i] = ye[i];
      xx += xs[i] * xs[i];
      yy += ys[i] * ys[i];
    }
    const double alpha = sqrt(xx) / (sqrt(yy) + ST_EPS);
    double mx = 0.0, my = 0.0;
#pragma unroll
    for (int i = 0; i < ST_SEG; ++i) {
      const double scaled = alpha * ys[i], ceiling = ST_CLIP * xs[i];
      ys[i] = scaled > ceiling ? ceiling : scaled;        // a NaN of the degraded row stays one (fmin would drop it)
      mx += xs[i];
      my += ys[i];
    }
    mx /= (double)ST_SEG;
    my /= (double)ST_SEG;
    xx = yy = 0.0;
#pragma unroll
    for (int i = 0; i < ST_SEG; ++i) {
      xs[i] -= mx;
      ys[i] -= my;
      xx += xs[i] * xs[i];
      yy += ys[i] * ys[i];
    }
    const double nx = sqrt(xx) + ST_EPS, ny = sqrt(yy) + ST_EPS;
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < ST_SEG; ++i) d += (xs[i] / nx) * (ys[i] / ny);
    acc[0] += d;
  }
  block_sum<kSequential, true>(acc, s_red);
  if (tid == 0) value[b] = acc[0] / (double)pairs;
}

// -------------------------------------------------------------------------------------------------------------------- SI-SDR
template <typename T>
__global__ __launch_bounds__(SM_THREADS) void si_sdr_kernel(const T* __restrict__ reference, const T* __restrict__ estimate,
                                                            double* __restrict__ out, int n) {
  __shared__ double s_red[2][SM_WAVES];
  const int tid = threadIdx.x;
  const T* s = reference + (long)blockIdx.x * n;
  const T* e = estimate + (long)blockIdx.x * n;
  double v[2] = {0.0, 0.0};
  for (int t = tid; t < n; t += SM_THREADS) {
    v[0] += (double)s[t];
    v[1] += (double)e[t];
  }
  block_sum<kSequential, true>(v, s_red);
  const double ms = v[0] / (double)n, me = v[1] / (double)n;
  v[0] = v[1] = 0.0;
  for (int t = tid; t < n; t += SM_THREADS) {
    const double a = (double)s[t] - ms, c = (double)e[t] - me;
    v[0] += a * a;
    v[1] += c * a;
  }
  block_sum<kSequential, true>(v, s_red);
  const double ss = v[0];
  if (!(ss > 0.0 && ss <= DBL_MAX)) {
    if (tid == 0) out[blockIdx.x] = NAN;
    return;
  }
  const double alpha = v[1] / ss;
  v[0] = v[1] = 0.0;
  for (int t = tid; t < n; t += SM_THREADS) {
    const double target = alpha * ((double)s[t] - ms), c = (double)e[t] - me;
    v[0] += target * target;
    v[1] += (target - c) * (target - c);
  }
  block_sum<kSequential, true>(v, s_red);
  if (tid != 0) return;
  double r;
  if (v[0] != v[0] || v[1] != v[1]) r = NAN;
  else if (v[1] == 0.0) r = INFINITY;
  else r = 10.0 * log10(v[0] / v[1]);
  out[blockIdx.x] = r;
}

// ----------------------------------------------------------------------------------------------------------------------- LSD
template <typename T>
__global__ __launch_bounds__(SM_THREADS) void lsd_kernel(const T* __restrict__ p, const T* __restrict__ q,
                                                         double* __restrict__ out, int F, int T_frames, double eps) {
  __shared__ double s_red[2][SM_WAVES];
  const long row = (long)blockIdx.x * F * T_frames;
  double v[2] = {0.0, 0.0};                // the frames' distances; how many entries were negative or not finite
  for (int t = threadIdx.x; t < T_frames; t += SM_THREADS) {
    double s = 0.0;
    for (int f = 0; f < F; ++f) {
      const double a = (double)p[row + (long)f * T_frames + t], c = (double)q[row + (long)f * T_frames + t];
      if (!(a >= 0.0 && a <= DBL_MAX && c >= 0.0 && c <= DBL_MAX)) v[1] += 1.0;
      const double d = 10.0 * log10((a + eps) / (c + eps));
      s += d * d;
    }
    v[0] += sqrt(s / (double)F);
  }
  block_sum<kSequential, true>(v, s_red);
  if (threadIdx.x == 0) out[blockIdx.x] = v[1] != 0.0 ? NAN : v[0] / (double)T_frames;
}

}  // namespace alvq

using namespace alvq;

static int sm_check_rows(const char* who, int B, int n, int min_n) {
  ALVQ_REQUIRE(B >= 1 && B <= SM_MAX_ROWS && n >= min_n && n <= SM_MAX_N, ALVQ_EINVAL,
               "%s: B=%d n=%d (need 1 <= B <= 65535, %d <= n <= 2^24)", who, B, n, min_n);
  return ALVQ_OK;
}

template <typename T>
static int resample_poly_launch(const char* who, const T* x, const double* h, double* y, int B, int n, int up, int down, int half,
                                void* stream) {
  ALVQ_REQUIRE(x && h && y, ALVQ_EINVAL, "%s: null pointer", who);
  const int rc = sm_check_rows(who, B, n, 1);
  if (rc != ALVQ_OK) return rc;
  ALVQ_REQUIRE(up >= 1 && down >= 1 && up <= SM_MAX_RATE && down <= SM_MAX_RATE && half >= 0 && half <= 10 * SM_MAX_RATE,
               ALVQ_EINVAL, "%s: up=%d down=%d half=%d (need 1 <= up, down <= 512, 0 <= half <= 5120)", who, up, down, half);
  const long n_out = ((long)n * up + down - 1) / down;
  ALVQ_REQUIRE(n_out <= INT_MAX, ALVQ_EINVAL, "%s: %ld output samples a row (need <= 2^31 - 1)", who, n_out);
  const dim3 grid((unsigned)((n_out + SM_THREADS - 1) / SM_THREADS), B);
  if (2 * half + 1 <= RS_LDS_TAPS)
    hipLaunchKernelGGL((resample_poly_kernel<T, true>), grid, dim3(SM_THREADS), 0, (hipStream_t)stream, x, h, y, n, n_out, up, down,
                       half);
  else
    hipLaunchKernelGGL((resample_poly_kernel<T, false>), grid, dim3(SM_THREADS), 0, (hipStream_t)stream, x, h, y, n, n_out, up, down,
                       half);
  return check_launch(who);
}

extern "C" int alvq_resample_poly_f32(const float* x, const double* h, double* y, int B, int n, int up, int down, int half,
                                      void* stream) {
  return resample_poly_launch("alvq_resample_poly_f32", x, h, y, B, n, up, down, half, stream);
}

extern "C" int alvq_resample_poly_f64(const double* x, const double* h, double* y, int B, int n, int up, int down, int half,
                                      void* stream) {
  return resample_poly_launch("alvq_resample_poly_f64", x, h, y, B, n, up, down, half, stream);
}

static int stoi_frame_count(int n) { return n >= ST_FRAME ? (n - ST_FRAME) / ST_HOP + 1 : 0; }

// the workspace: B nf frame energies, 2 * 15 * B nf band envelopes (doubles), B nf kept-frame indices (ints)
extern "C" int64_t alvq_stoi_workspace_bytes(int B, int n) {
  if (B < 1 || B > SM_MAX_ROWS || n < 2 || n > SM_MAX_N) return -1;
  const int64_t frames = (int64_t)B * stoi_frame_count(n);
  return frames * (8 + 2 * ST_BANDS * 8 + 4) + 256;
}

extern "C" int alvq_stoi_f64(const double* clean, const double* degraded, const int* band_lo_host, const int* band_hi_host,
                             double* value, int* kept_frames, int* status, void* workspace, int B, int n, void* stream) {
  const char* who = "alvq_stoi_f64";
  ALVQ_REQUIRE(clean && degraded && band_lo_host && band_hi_host && value && kept_frames && status && workspace, ALVQ_EINVAL,
               "%s: null pointer", who);
  const int rc = sm_check_rows(who, B, n, 2);
  if (rc != ALVQ_OK) return rc;
  StoiBands bands;
  int first = INT_MAX, last = 0;
  for (int j = 0; j < ST_BANDS; ++j) {
    const int lo = band_lo_host[j], hi = band_hi_host[j];
    ALVQ_REQUIRE(lo >= 0 && lo < hi && hi <= ST_NFFT / 2 + 1, ALVQ_EINVAL, "%s: band %d covers bins [%d, %d) (need 0 <= lo < hi <= 257)",
                 who, j, lo, hi);
    bands.lo[j] = lo;
    bands.hi[j] = hi;
    first = lo < first ? lo : first;
    last = hi > last ? hi : last;
  }
  ALVQ_REQUIRE(last - first <= SM_THREADS, ALVQ_EINVAL, "%s: the bands span %d bins (need <= 256)", who, last - first);
  bands.first = first;
  bands.count = last - first;
  const int nf = stoi_frame_count(n);
  const long frames = (long)B * nf;
  double* energy = (double*)workspace;
  double* env = energy + frames;
  int* kept = (int*)(env + 2 * ST_BANDS * frames);
  hipStream_t s = (hipStream_t)stream;
  if (nf > 0) {
    hipLaunchKernelGGL(stoi_energy_kernel, dim3((nf + SM_WAVES - 1) / SM_WAVES, B), dim3(SM_THREADS), 0, s, clean, energy, n, nf);
    int rc1 = check_launch(who);
    if (rc1 != ALVQ_OK) return rc1;
  }
  hipLaunchKernelGGL(stoi_mask_kernel, dim3(B), dim3(SM_THREADS), 0, s, energy, kept, kept_frames, status, nf);
  int rc2 = check_launch(who);
  if (rc2 != ALVQ_OK) return rc2;
  if (nf > 0) {
    hipLaunchKernelGGL(stoi_envelope_kernel, dim3(nf, B), dim3(SM_THREADS), 0, s, clean, degraded, kept, kept_frames, env, bands, n,
                       nf);
    rc2 = check_launch(who);
    if (rc2 != ALVQ_OK) return rc2;
  }
  hipLaunchKernelGGL(stoi_correlate_kernel, dim3(B), dim3(SM_THREADS), 0, s, env, kept_frames, status, value, nf);
  return check_launch(who);
}

template <typename T>
static int si_sdr_launch(const char* who, const T* reference, const T* estimate, double* out, int B, int n, void* stream) {
  ALVQ_REQUIRE(reference && estimate && out, ALVQ_EINVAL, "%s: null pointer", who);
  const int rc = sm_check_rows(who, B, n, 2);
  if (rc != ALVQ_OK) return rc;
  hipLaunchKernelGGL(si_sdr_kernel<T>, dim3(B), dim3(SM_THREADS), 0, (hipStream_t)stream, reference, estimate, out, n);
  return check_launch(who);
}

extern "C" int alvq_si_sdr_f32(const float* reference, const float* estimate, double* out, int B, int n, void* stream) {
  return si_sdr_launch("alvq_si_sdr_f32", reference, estimate, out, B, n, stream);
}

extern "C" int alvq_si_sdr_f64(const double* reference, const double* estimate, double* out, int B, int n, void* stream) {
  return si_sdr_launch("alvq_si_sdr_f64", reference, estimate, out, B, n, stream);
}

template <typename T>
static int lsd_launch(const char* who, const T* p, const T* q, double* out, int B, int F, int T_frames, double eps, void* stream) {
  ALVQ_REQUIRE(p && q && out, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(B >= 1 && B <= SM_MAX_ROWS && F >= 1 && T_frames >= 1 && (long)F * T_frames <= (1L << 30), ALVQ_EINVAL,
               "%s: B=%d F=%d T=%d (need 1 <= B <= 65535, F, T >= 1, F T <= 2^30)", who, B, F, T_frames);
  ALVQ_REQUIRE(std::isfinite(eps) && eps >= 0.0, ALVQ_EINVAL, "%s: eps=%g must be finite and >= 0", who, eps);
  hipLaunchKernelGGL(lsd_kernel<T>, dim3(B), dim3(SM_THREADS), 0, (hipStream_t)stream, p, q, out, F, T_frames, eps);
  return check_launch(who);
}

extern "C" int alvq_lsd_f32(const float* p, const float* q, double* out, int B, int F, int T, double eps, void* stream) {
  return lsd_launch("alvq_lsd_f32", p, q, out, B, F, T, eps, stream);
}

extern "C" int alvq_lsd_f64(const double* p, const double* q, double* out, int B, int F, int T, double eps, void* stream) {
  return lsd_launch("alvq_lsd_f64", p, q, out, B, F, T, eps, stream);
}
