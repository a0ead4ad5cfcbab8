// The framed direct DFT that the STFT (stft.hip), the inverse STFT and Griffin-Lim (istft.hip) share: how a waveform is cut into
// frames, windowed and transformed is decided here and nowhere else.
//
// One workgroup of 256 threads = DFT_FT consecutive frames of one item.  Dynamic LDS is [cs | sn | body]: a cos/sin table of
// n_fft entries each (built in fp64, stored as R) and the staged frames (forward) or one-sided spectra (inverse).  Forward, thread
// k accumulates bin k of all DFT_FT frames (frame samples are LDS broadcasts); every sum runs in a fixed order, so a result is
// bitwise reproducible.
//
// Two windows live here and are not interchangeable, bit for bit: load_frames forms the periodic Hann window from the ROUNDED
// table, (R)0.5 - (R)0.5 * cs[n] (what the forward kernels have always done, and what the tests' tolerance model describes);
// hann<R> is computed in fp64 and rounded once (the inverse kernels).
#pragma once
#include "alvq_common.h"

namespace alvq {

constexpr int DFT_FT = 8;  // frames per workgroup

template <typename R>
__device__ __forceinline__ void fill_twiddles(R* cs, R* sn, int N, int tid) {
  for (int j = tid; j < N; j += 256) {
    const double ang = 2.0 * (double)j / (double)N;
    cs[j] = (R)cospi(ang);
    sn[j] = (R)sinpi(ang);
  }
}

template <typename R>
__device__ __forceinline__ R hann(int n, int N) {
  return (R)(0.5 - 0.5 * cospi(2.0 * (double)n / (double)N));  // periodic Hann
}

// workgroup blockIdx.x of dft_grid(B, T) -> item b and its first frame t0
struct FrameTile {
  int b, t0;
};
__device__ __forceinline__ FrameTile frame_tile(int T) {
  const int ttiles = (T + DFT_FT - 1) / DFT_FT;
  const int b = blockIdx.x / ttiles, t0 = (blockIdx.x % ttiles) * DFT_FT;
  return FrameTile{b, t0};
}

// fr[f][n] = wv[reflect(t * hop + n - N/2)] * w[n] for the frames t = t0 + f < T (center=True, reflect padding; S > N/2, so one
// reflection suffices), 0 for the frames at or beyond T.  Reads cs: a barrier after fill_twiddles comes first.
template <typename R>
__device__ __forceinline__ void load_frames(R* fr, const R* cs, const R* wv, int S, int N, int hop, int T, int t0, int tid) {
  for (int e = tid; e < DFT_FT * N; e += 256) {
    const int f = e / N, n = e - f * N;
    const int t = t0 + f;
    R v = 0;
    if (t < T) {
      int i = t * hop + n - N / 2;
      if (i < 0) i = -i;
      if (i >= S) i = 2 * (S - 1) - i;
      const R w = (R)0.5 - (R)0.5 * cs[n];  // periodic Hann, from the rounded table
      v = wv[i] * w;
    }
    fr[e] = v;
  }
}

// The one-sided DFT of the staged frames: X[k] = sum_n fr[f][n] (cos - i sin)(2 pi k n / N), n ascending, for the bins
// k = tid, tid + 256, ... <= N/2.  tail(k, t, re, im) receives bin k of every frame t = t0 + f < T.
template <typename R, typename Tail>
__device__ __forceinline__ void forward_dft(const R* cs, const R* sn, const R* fr, int N, int T, int t0, int tid, Tail tail) {
  const int F = N / 2 + 1;
  for (int k = tid; k < F; k += 256) {
    R re[DFT_FT], im[DFT_FT];
#pragma unroll
    for (int f = 0; f < DFT_FT; ++f) re[f] = im[f] = 0;
    int idx = 0;
    for (int n = 0; n < N; ++n) {
      const R c = cs[idx], s = sn[idx];
#pragma unroll
      for (int f = 0; f < DFT_FT; ++f) {
        const R x = fr[f * N + n];
        re[f] += x * c;
        im[f] -= x * s;
      }
      idx += k;
      if (idx >= N) idx -= N;
    }
#pragma unroll
    for (int f = 0; f < DFT_FT; ++f)
      if (t0 + f < T) tail(k, t0 + f, re[f], im[f]);
  }
}

// ---- host side: one size cap, one grid, and the two dynamic-LDS byte counts side by side
template <typename R>
constexpr int dft_max_n_fft() {
  return 2048 * (int)sizeof(float) / (int)sizeof(R);  // 2048 in fp32, 1024 in fp64: at most 80 KB of table + body
}

inline dim3 dft_grid(int B, int T) { return dim3(B * ((T + DFT_FT - 1) / DFT_FT)); }

// [cs | sn | DFT_FT frames of n_fft samples]
template <typename R>
constexpr size_t dft_forward_lds(int n_fft) {
  return (size_t)(2 + DFT_FT) * n_fft * sizeof(R);
}
// [cs | sn | DFT_FT one-sided spectra of n_fft/2 + 1 interleaved bins]: 2 * DFT_FT elements more than the forward count
template <typename R>
constexpr size_t dft_inverse_lds(int n_fft) {
  return (size_t)(2 * n_fft + DFT_FT * 2 * (n_fft / 2 + 1)) * sizeof(R);
}
constexpr int DFT_LDS_LIMIT = 96 * 1024;  // hipFuncAttributeMaxDynamicSharedMemorySize of every kernel built on this header

}  // namespace alvq
