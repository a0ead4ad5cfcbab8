// Inverse STFT and Griffin-Lim phase reconstruction: the way back from the front end's spectrograms to a waveform
// (torchaudio InverseSpectrogram(n_fft, hop, center=True, pad=0, normalized=True) and torchaudio.functional.griffinlim).
//
// Three kernels, every one a fixed-order sum (no atomics), so a result is bitwise reproducible:
//   irfft_frames_kernel  one workgroup = 8 frames of one item; the 8 spectra and a cos/sin table (built in fp64) live in LDS,
//                        thread n sums the one-sided inverse DFT of sample n of all 8 frames and writes it windowed into the
//                        frame workspace (B, T, n_fft).
//   ola_gather_kernel    one thread per output sample: sums the <= ceil(n_fft/hop) windowed frames that cover it, in
//                        ascending frame order, and divides by the overlap-added w^2 envelope (computed in place).
//   stft_project_kernel  Griffin-Lim's forward STFT (the framing and transform of csrc/stft.hip, both from dft_frames.h) with
//                        the projection as its tail: it reads tprev, writes rebuilt over it, and writes the next mag * angles
//                        for the inverse.  No separate elementwise pass over the spectra.
// Griffin-Lim enqueues 3 launches per iteration + 2 on one stream: a linear chain, capturable in a single-stream graph.
#include <algorithm>
#include <cmath>
#include <vector>

#include "dft_frames.h"

namespace alvq {

// frames[b][t][n] = scale * w[n] * (X0.re + (-1)^n X_{N/2}.re + 2 sum_{k=1}^{N/2-1} (Xk.re cos - Xk.im sin)(2 pi k n / N)),
// X = spec[b][:, t] (interleaved), or mag[b][:, t] * spec[b][:, t] when mag is given (Griffin-Lim's first inverse).
// As irfft, the imaginary parts of the DC and Nyquist bins are ignored.
template <typename R>
__global__ __launch_bounds__(256) void irfft_frames_kernel(const R* spec, const R* mag, R* frames, int N, int T, R scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
  R* sm = (R*)sm_raw;
  const int F = N / 2 + 1;
  R* cs = sm;               // [N]
  R* sn = sm + N;           // [N]
  R* xs = sm + 2 * N;       // [DFT_FT][F][2]
  const int tid = threadIdx.x;
  const FrameTile tile = frame_tile(T);
  const int b = tile.b, t0 = tile.t0;
  fill_twiddles(cs, sn, N, tid);
  for (int e = tid; e < DFT_FT * F; e += 256) {
    const int f = e / F, k = e - f * F;
    const int t = t0 + f;
    R re = 0, im = 0;
    if (t < T) {
      const long o = ((long)b * F + k) * T + t;
      re = spec[2 * o];
      im = spec[2 * o + 1];
      if (mag) {
        const R m = mag[o];
        re *= m;
        im *= m;
      }
    }
    xs[2 * e] = re;
    xs[2 * e + 1] = im;
  }
  __syncthreads();
  for (int n = tid; n < N; n += 256) {
    R acc[DFT_FT];
    const R sgn = (n & 1) ? (R)-1 : (R)1;
#pragma unroll
    for (int f = 0; f < DFT_FT; ++f) acc[f] = 0;
    int idx = n;
    for (int k = 1; k < F - 1; ++k) {
      const R c = cs[idx], s = sn[idx];
#pragma unroll
      for (int f = 0; f < DFT_FT; ++f) {
        const R* x = xs + 2 * (f * F + k);
        acc[f] += x[0] * c - x[1] * s;
      }
      idx += n;
      if (idx >= N) idx -= N;
    }
    const R w = hann<R>(n, N) * scale;
#pragma unroll
    for (int f = 0; f < DFT_FT; ++f)
      if (t0 + f < T) {
        const R v = xs[2 * f * F] + sgn * xs[2 * (f * F + F - 1)] + (R)2 * acc[f];
        frames[((long)b * T + t0 + f) * N + n] = v * w;
      }
  }
}

// wave[b][i] = sum_t frames[b][t][p - t*hop] / sum_t w[p - t*hop]^2, p = i + N/2 (center=True), over the frames t that cover
// p, ascending.  Past the overlap-added signal (p >= N + hop*(T-1): an explicit length longer than it) the output is 0.
// The envelope is > 1e-11 wherever a frame covers p (checked on the host before launch).
template <typename R>
__global__ __launch_bounds__(256) void ola_gather_kernel(const R* frames, R* wave, int N, int hop, int T, int length) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= length) return;
  const int p = i + N / 2;
  R v = 0;
  if (p < N + hop * (T - 1)) {
    const int t_lo = p >= N ? (p - N) / hop + 1 : 0;
    const int t_hi = min(T - 1, p / hop);
    const R* fb = frames + (long)b * T * N;
    R s = 0, env = 0;
    for (int t = t_lo; t <= t_hi; ++t) {
      const int n = p - t * hop;
      const R w = hann<R>(n, N);
      s += fb[(long)t * N + n];
      env += w * w;
    }
    v = s / env;
  }
  wave[(long)b * length + i] = v;
}

// One Griffin-Lim projection.  rebuilt = STFT(wave) (center=True, reflect pad, periodic Hann, one-sided, unnormalised);
// a = rebuilt - coef * tprev (tprev = 0 when first); tprev <- rebuilt; next[.] = mag * a / (|a| + 1e-16).
template <typename R>
__global__ __launch_bounds__(256) void stft_project_kernel(const R* wave, const R* mag, R* tprev, R* next, int S, int N, int hop,
                                                           int T, R coef, int first) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
  R* sm = (R*)sm_raw;
  R* cs = sm;               // [N]
  R* sn = sm + N;           // [N]
  R* fr = sm + 2 * N;       // [DFT_FT][N]
  const int tid = threadIdx.x;
  const FrameTile tile = frame_tile(T);
  const int b = tile.b, t0 = tile.t0;
  const int F = N / 2 + 1;
  fill_twiddles(cs, sn, N, tid);
  __syncthreads();
  load_frames(fr, cs, wave + (long)b * S, S, N, hop, T, t0, tid);
  __syncthreads();
  forward_dft(cs, sn, fr, N, T, t0, tid, [=](int k, int t, R re, R im) {
    const long o = ((long)b * F + k) * T + t;
    R ar = re, ai = im;
    if (!first) {
      ar -= coef * tprev[2 * o];
      ai -= coef * tprev[2 * o + 1];
    }
    tprev[2 * o] = re;
    tprev[2 * o + 1] = im;
    const R inv = (R)1 / (sqrt(ar * ar + ai * ai) + (R)1e-16);
    const R m = mag[o];
    next[2 * o] = m * (ar * inv);
    next[2 * o + 1] = m * (ai * inv);
  });
}

}  // namespace alvq

using namespace alvq;

static double wsum_of(int N) {
  double s = 0.0;
  for (int j = 0; j < N; ++j) {
    const double w = 0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)N);
    s += w * w;
  }
  return s;
}

// The checks every entry point shares: sizes as stft_launch, and the NOLA condition of torch.istft (overlap-added w^2 > 1e-11
// over the output samples that the overlap-added signal covers).  Host only: no launch, no sync.
template <typename R>
static int istft_check(int B, int T, int n_fft, int hop, int length, const char* who) {
  ALVQ_REQUIRE(B > 0 && T > 0 && hop > 0 && n_fft >= 4 && n_fft % 2 == 0 && length > 0, ALVQ_EINVAL,
               "%s: bad dims (B=%d T=%d n_fft=%d hop=%d length=%d; even n_fft >= 4)", who, B, T, n_fft, hop, length);
  ALVQ_REQUIRE(n_fft <= dft_max_n_fft<R>(), ALVQ_EINVAL, "%s: n_fft=%d too large", who, n_fft);
  ALVQ_REQUIRE((long)n_fft + (long)hop * (T - 1) < (1L << 30), ALVQ_EINVAL, "%s: signal too long", who);
  const int total = n_fft + hop * (T - 1), p0 = n_fft / 2, p1 = std::min(p0 + length, total);
  std::vector<double> env(total, 0.0);
  for (int t = 0; t < T; ++t)
    for (int n = 0; n < n_fft; ++n) {
      const double w = 0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)n_fft);
      env[(size_t)t * hop + n] += w * w;
    }
  for (int p = p0; p < p1; ++p)
    ALVQ_REQUIRE(env[p] > 1e-11, ALVQ_EINVAL, "%s: window overlap-add is zero at sample %d (NOLA fails for n_fft=%d hop=%d)", who,
                 p - p0, n_fft, hop);
  return 0;
}

template <typename R>
static void enqueue_inverse(const R* spec, const R* mag, R* wave, R* frames, int B, int T, int n_fft, int hop, int length, R scale,
                            hipStream_t s) {
  hipLaunchKernelGGL(irfft_frames_kernel<R>, dft_grid(B, T), dim3(256), dft_inverse_lds<R>(n_fft), s, spec, mag, frames, n_fft, T,
                     scale);
  hipLaunchKernelGGL(ola_gather_kernel<R>, dim3((length + 255) / 256, B), dim3(256), 0, s, (const R*)frames, wave, n_fft, hop, T,
                     length);
}

// once per device and precision (a launch site that sets the attribute on every call would do so inside a graph capture too)
template <typename R>
static void set_lds_limits() {
  static DeviceOnce attr;
  if (!attr.need()) return;
  (void)hipFuncSetAttribute((const void*)irfft_frames_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, DFT_LDS_LIMIT);
  (void)hipFuncSetAttribute((const void*)stft_project_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, DFT_LDS_LIMIT);
}

template <typename R>
static int istft_launch(const R* spec, R* wave, R* workspace, int B, int T, int n_fft, int hop, int length, void* stream,
                        const char* who) {
  ALVQ_REQUIRE(spec && wave && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  if (int rc = istft_check<R>(B, T, n_fft, hop, length, who)) return rc;
  set_lds_limits<R>();
  // torch.istft(spec * sqrt(sum w^2)): the 1/n_fft of the inverse DFT and the normalisation folded into one factor
  const R scale = (R)(sqrt(wsum_of(n_fft)) / (double)n_fft);
  enqueue_inverse<R>(spec, (const R*)nullptr, wave, workspace, B, T, n_fft, hop, length, scale, (hipStream_t)stream);
  return check_launch(who);
}

template <typename R>
static int64_t gl_workspace(int B, int n_fft, int T) {
  const int64_t F = n_fft / 2 + 1;
  return (4 * (int64_t)B * F * T + (int64_t)B * T * n_fft) * (int64_t)sizeof(R);
}

template <typename R>
static int griffin_lim_launch(const R* mag, const R* angles, R* wave, void* workspace, int B, int T, int n_fft, int hop, int length,
                              int n_iter, double momentum, void* stream, const char* who) {
  ALVQ_REQUIRE(mag && angles && wave && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  if (int rc = istft_check<R>(B, T, n_fft, hop, length, who)) return rc;
  ALVQ_REQUIRE(n_iter >= 0 && momentum >= 0.0 && momentum < 1.0, ALVQ_EINVAL, "%s: n_iter=%d momentum=%g (need n_iter >= 0, "
               "0 <= momentum < 1)", who, n_iter, momentum);
  ALVQ_REQUIRE(n_iter == 0 || (1 + length / hop == T && length > n_fft / 2), ALVQ_EINVAL,
               "%s: the STFT of a %d-sample waveform has %d frames, not T=%d (reflect padding also needs length > n_fft/2)", who,
               length, 1 + length / hop, T);
  set_lds_limits<R>();
  const int F = n_fft / 2 + 1;
  const size_t spec_elems = (size_t)2 * B * F * T;
  R* next = (R*)workspace;            // mag * angles, the spectrum the next inverse reads
  R* tprev = next + spec_elems;       // the previous iteration's rebuilt STFT
  R* frames = tprev + spec_elems;     // (B, T, n_fft) windowed inverse frames
  hipStream_t s = (hipStream_t)stream;
  // torchaudio runs on mag * sqrt(sum w^2) with an unnormalised window; the factor is folded into the inverse's scale, which the
  // 1e-16 of the phase normalisation does not see: rebuilt is the unnormalised STFT of the same waveform either way
  const R scale = (R)(sqrt(wsum_of(n_fft)) / (double)n_fft);
  const R coef = (R)(momentum / (1.0 + momentum));
  // the projection is launched with the inverse's byte count, 2 * DFT_FT elements above what its frames need: one number for
  // the whole chain (the smaller one could move an occupancy boundary of the projection that has not been measured)
  const size_t lds = dft_inverse_lds<R>(n_fft);
  enqueue_inverse<R>(angles, mag, wave, frames, B, T, n_fft, hop, length, scale, s);
  for (int it = 0; it < n_iter; ++it) {
    hipLaunchKernelGGL(stft_project_kernel<R>, dft_grid(B, T), dim3(256), lds, s, (const R*)wave, mag, tprev, next, length, n_fft,
                       hop, T, coef, (int)(it == 0));
    enqueue_inverse<R>(next, (const R*)nullptr, wave, frames, B, T, n_fft, hop, length, scale, s);
  }
  return check_launch(who);
}

extern "C" int alvq_istft_f32(const float* spec, float* wave, float* workspace, int B, int T, int n_fft, int hop, int length,
                              void* stream) {
  return istft_launch<float>(spec, wave, workspace, B, T, n_fft, hop, length, stream, "alvq_istft_f32");
}

extern "C" int alvq_istft_f64(const double* spec, double* wave, double* workspace, int B, int T, int n_fft, int hop, int length,
                              void* stream) {
  return istft_launch<double>(spec, wave, workspace, B, T, n_fft, hop, length, stream, "alvq_istft_f64");
}

extern "C" int64_t alvq_griffin_lim_workspace_bytes(int B, int T, int n_fft, int elem_bytes) {
  if (B <= 0 || T <= 0 || n_fft < 4 || n_fft % 2) return -1;
  if (elem_bytes == 4) return gl_workspace<float>(B, n_fft, T);
  if (elem_bytes == 8) return gl_workspace<double>(B, n_fft, T);
  return -1;
}

extern "C" int alvq_griffin_lim_f32(const float* mag, const float* angles, float* wave, void* workspace, int B, int T, int n_fft,
                                    int hop, int length, int n_iter, double momentum, void* stream) {
  return griffin_lim_launch<float>(mag, angles, wave, workspace, B, T, n_fft, hop, length, n_iter, momentum, stream,
                                   "alvq_griffin_lim_f32");
}

extern "C" int alvq_griffin_lim_f64(const double* mag, const double* angles, double* wave, void* workspace, int B, int T, int n_fft,
                                    int hop, int length, int n_iter, double momentum, void* stream) {
  return griffin_lim_launch<double>(mag, angles, wave, workspace, B, T, n_fft, hop, length, n_iter, momentum, stream,
                                    "alvq_griffin_lim_f64");
}
