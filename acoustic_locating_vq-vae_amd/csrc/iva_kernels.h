// The one owner of what the determined separators share (device kernels and their host-side helpers; included by csrc/iva.hip
// and csrc/ilrma.hip): the bin check and start of W, the weighted covariances, the wave-a-bin elimination with the iterative-
// projection update, and the projection back onto the reference microphone.  What each kernel does and why it is laid out as
// it is: the header comment of csrc/iva.hip.  The two users differ in the covariance's weight alone:
//   AuxIVA   phi[b, k, t], the same in every bin:   iva_cov_kernel(..., row_stride = T, bin_stride = 0)
//   ILRMA    1 / R[b, k, f, t]:                     iva_cov_kernel(..., row_stride = F T, bin_stride = T)
// and in ILRMA's scaling of row k of W by 1 / sqrt(lam[b, k]) as the update loads it (iva_solve_kernel<D, true>); with
// SCALED = false the kernel never touches lam.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>

#include "array_wave.h"

namespace alvq {

constexpr int IVA_THREADS = 256;
constexpr int IVA_WAVES = IVA_THREADS / kWave;
constexpr int IVA_TILE = 64;               // the frames of a workgroup of iva_activity_kernel: a lane each, in every wave
constexpr int IVA_MAX_ITERATIONS = 256;

constexpr int IVA_BAD_INPUT = 1;           // a non-finite value in the bin, or a bin of zeros
constexpr int IVA_BAD_SOLVE = 2;           // a pivot or Re(w^H V w) that is 0 (<= 0) or not finite, or a singular W at the end

constexpr int IVA_LAPLACE = 0, IVA_GAUSS = 1;

// M z = rhs for every column of rhs at once, on the wave's layout: lane 8 r + c holds entry (r, c) of M and of rhs (a single
// right-hand side is held in every column).  Gaussian elimination with partial pivoting, column j = 0 .. D - 1: the pivot is the
// entry of the largest |z|^2 = re^2 + im^2 among the rows i >= j, the lowest row winning ties; rows j and the pivot's are
// exchanged; row r > j loses l = M[r][j] / pivot times row j.  Back substitution j = D - 1 .. 0.  The solution replaces rhs.
// IVA_BAD_SOLVE where a pivot's |z|^2 is 0 or not finite (what the lanes then hold is not used).  The lanes outside the D x D
// block hold zeros and only ever read each other.
template <int D>
__device__ __forceinline__ int iva_solve(double2& m, double2& rhs, int r, int c) {
  int fail = 0;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const double mag = m.x * m.x + m.y * m.y;
    double best = __shfl(mag, 9 * j, 64);
    int p = j;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      const double v = __shfl(mag, 8 * i + j, 64);
      if (v > best) {
        best = v;
        p = i;
      }
    }
    if (!(best > 0.0 && best <= DBL_MAX)) fail = IVA_BAD_SOLVE;
    const int src = r == j ? p : (r == p ? j : r);
    m = cshfl(m, 8 * src + c);
    rhs = cshfl(rhs, 8 * src + c);
    const double2 piv = cshfl(m, 9 * j), mrj = cshfl(m, 8 * r + j), mjc = cshfl(m, 8 * j + c);
    const double2 bjc = cshfl(rhs, 8 * j + c);
    if (r > j) {
      const double2 l = cdiv(mrj, piv);
      const double2 pm = cmul(l, mjc), pb = cmul(l, bjc);
      if (c > j) {
        m.x -= pm.x;
        m.y -= pm.y;
      } else if (c == j) {
        m = make_double2(0.0, 0.0);
      }
      rhs.x -= pb.x;
      rhs.y -= pb.y;
    }
  }
#pragma unroll
  for (int j = D - 1; j >= 0; --j) {
    const double2 piv = cshfl(m, 9 * j), bjc = cshfl(rhs, 8 * j + c), mrj = cshfl(m, 8 * r + j);
    const double2 z = cdiv(bjc, piv);
    if (r == j) {
      rhs = z;
    } else if (r < j) {
      const double2 pz = cmul(mrj, z);
      rhs.x -= pz.x;
      rhs.y -= pz.y;
    }
  }
  return fail;
}

// -------------------------------------------------------------------------------------------------------------------- check
template <typename R>
__global__ __launch_bounds__(IVA_THREADS) void iva_check_kernel(const void* X, const double2* W0, double2* W, int* status, long nbins,
                                                                 int D, int F, int T) {
  typedef typename Cplx<R>::type C;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long chan_stride = (long)F * T;
  for (long bin = (long)blockIdx.x * IVA_WAVES + wv; bin < nbins; bin += (long)gridDim.x * IVA_WAVES) {
    const int b = (int)(bin / F), f = (int)(bin % F);
    const C* xg = (const C*)X + ((long)b * D * F + f) * T;
    int bad = 0, any = 0;
    for (int d = 0; d < D; ++d)
      for (int t = lane; t < T; t += kWave) {
        const C v = xg[d * chan_stride + t];
        const double re = (double)v.x, im = (double)v.y;
        if (!is_finite(re) || !is_finite(im)) bad = 1;
        if (re != 0.0 || im != 0.0) any = 1;
      }
    bad = wave_or(bad);
    any = wave_or(any);
    const int st = (bad || !any) ? IVA_BAD_INPUT : 0;
    if (lane < D * D) {
      double2 w = make_double2(lane / D == lane % D ? 1.0 : 0.0, 0.0);
      if (!st && W0) w = W0[bin * (D * D) + lane];
      W[bin * (D * D) + lane] = w;
    }
    if (lane == 0) status[bin] = st;
  }
}

// --------------------------------------------------------------------------------------------------------------- covariance
// The weights of source k in bin (b, f) are the T values at Phi + (b D + k) row_stride + f bin_stride.
template <typename R, int D>
__global__ __launch_bounds__(IVA_THREADS) void iva_cov_kernel(const void* X, const double* Phi, const int* status, double2* V,
                                                              long nbins, int F, int T, long row_stride, long bin_stride) {
  typedef typename Cplx<R>::type C;
  constexpr int K = D * D;                             // D real diagonal sums and D (D - 1) / 2 complex ones below it
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long chan_stride = (long)F * T;
  // the grid is capped: a wave strides over its (bin, k) pairs, whole, and meets no barrier anywhere
  for (long e = (long)blockIdx.x * IVA_WAVES + wv; e < nbins * D; e += (long)gridDim.x * IVA_WAVES) {
    const long bin = e / D;
    const int k = (int)(e - bin * D);
    if (status[bin] != 0) continue;
    const int b = (int)(bin / F), f = (int)(bin % F);
    const C* xg = (const C*)X + ((long)b * D * F + f) * T;
    const double* phi = Phi + ((long)b * D + k) * row_stride + f * bin_stride;

    double acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n) acc[n] = 0.0;
    for (int t = lane; t < T; t += kWave) {
      C v[D];
#pragma unroll
      for (int d = 0; d < D; ++d) v[d] = xg[d * chan_stride + t];
      const double ph = phi[t];
      double2 x[D];
#pragma unroll
      for (int d = 0; d < D; ++d) x[d] = make_double2((double)v[d].x, (double)v[d].y);
      // a frame's term c = x_i conj(x_j): re = fma(x_i.im, x_j.im, x_i.re x_j.re), im = x_i.im x_j.re - x_i.re x_j.im (two
      // rounded products: exactly 0 where x_i = x_j); then acc = fma(phi, c, acc).  The diagonal has the real part alone.
      int n = 0;
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          const double re = fma(x[i].y, x[j].y, x[i].x * x[j].x);
          acc[n] = fma(ph, re, acc[n]);
          ++n;
          if (j < i) {
            const double im = x[i].y * x[j].x - x[i].x * x[j].y;
            acc[n] = fma(ph, im, acc[n]);
            ++n;
          }
        }
    }
#pragma unroll
    for (int n = 0; n < K; ++n) acc[n] = wave_sum(acc[n]);
    double re = 0.0, im = 0.0;                         // lane e = i D + j picks its entry; the divisions come after the choice
    int n = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const double sr = acc[n++];
        const double si = j < i ? acc[n++] : 0.0;
        if (lane == i * D + j) {
          re = sr;
          im = si;
        }
        if (j < i && lane == j * D + i) {
          re = sr;
          im = -si;                                    // the exact conjugate: a division keeps the sign
        }
      }
    if (lane < D * D) V[e * (D * D) + lane] = make_double2(re / (double)T, (lane / D == lane % D) ? 0.0 : im / (double)T);
  }
}

// -------------------------------------------------------------------------------------------------------------------- solve
// SCALED: row r of the bin's W is divided by sqrt(lam[b D + r]), part by part, as it is loaded (ILRMA's normalisation).
template <int D, bool SCALED = false>
__global__ __launch_bounds__(IVA_THREADS) void iva_solve_kernel(const double2* Vg, double2* W, int* status, long nbins,
                                                                const double* lam = nullptr, int F = 1) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane >> 3, c = lane & 7;
  const bool in = r < D && c < D;
  const int at = in ? r * D + c : 0;                   // a lane outside the block loads entry 0 and drops it
  const double2 zero = make_double2(0.0, 0.0);
  // the grid is capped: a wave strides over its bins, whole, and meets no barrier anywhere
  for (long bin = (long)blockIdx.x * IVA_WAVES + wv; bin < nbins; bin += (long)gridDim.x * IVA_WAVES) {
    if (status[bin] != 0) continue;
    double2 w = W[bin * (D * D) + at];
    if (SCALED) {
      const double s = sqrt(lam[(bin / F) * D + (in ? r : 0)]);
      w = make_double2(w.x / s, w.y / s);
    }
    if (!in) w = zero;
    int fail = 0;
    for (int k = 0; k < D && !fail; ++k) {             // `fail` is the same in every lane
      const double2* V = Vg + (bin * D + k) * (D * D);
      double2 m = zero;                                // (W V_k)[r][c], j rising from the first product
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 wrj = cshfl(w, 8 * r + j);
        const double2 q = cmul(wrj, V[in ? j * D + c : 0]);
        m = j == 0 ? q : make_double2(m.x + q.x, m.y + q.y);
      }
      if (!in) m = zero;
      double2 sol = make_double2(r == k ? 1.0 : 0.0, 0.0);            // e_k in every column
      fail = iva_solve<D>(m, sol, r, c);               // the lanes of row r hold w_r
      const double2 wc = cshfl(sol, 8 * c);
      const double2 term = in ? cmul(V[at], wc) : zero;
      double2 vw = zero;                               // (V_k w)[r], c rising from the first product
#pragma unroll
      for (int cc = 0; cc < D; ++cc) {
        const double2 q = cshfl(term, 8 * r + cc);
        vw = cc == 0 ? q : make_double2(vw.x + q.x, vw.y + q.y);
      }
      const double qr = sol.x * vw.x + sol.y * vw.y;                  // Re(conj(w_r) (V_k w)_r)
      double q = 0.0;
#pragma unroll
      for (int rr = 0; rr < D; ++rr) {
        const double v = __shfl(qr, 8 * rr, 64);
        q = rr == 0 ? v : q + v;
      }
      if (!(q > 0.0 && q <= DBL_MAX)) fail = IVA_BAD_SOLVE;
      const double s = sqrt(q);
      if (!fail && in && r == k) w = make_double2(wc.x / s, -(wc.y / s));
    }
    if (fail) w = make_double2(r == c ? 1.0 : 0.0, 0.0);
    if (in) W[bin * (D * D) + r * D + c] = w;
    if (fail && lane == 0) status[bin] = IVA_BAD_SOLVE;
  }
}

// ------------------------------------------------------------------------------------------------------------------ project
template <typename R, int D>
__global__ __launch_bounds__(IVA_THREADS) void iva_project_kernel(const void* X, double2* W, void* Y, int* status, long nbins, int F,
                                                                  int T, int ref) {
  typedef typename Cplx<R>::type C;
  __shared__ double2 Ws[D * D];
  __shared__ double2 As[D];
  __shared__ int s_pass;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane >> 3, c = lane & 7;
  const bool in = r < D && c < D;
  const int at = in ? r * D + c : 0;               // a lane outside the block loads entry 0 and drops it
  const long chan_stride = (long)F * T;
  const double2 zero = make_double2(0.0, 0.0);
  for (long bin = blockIdx.x; bin < nbins; bin += gridDim.x) {
    const int b = (int)(bin / F), f = (int)(bin % F);
    if (wv == 0) {
      int st = status[bin];
      if (st == 0) {
        double2 w = W[bin * (D * D) + at];
        if (!in) w = zero;
        double2 m = w, inv = make_double2(in && r == c ? 1.0 : 0.0, 0.0);
        if (iva_solve<D>(m, inv, r, c)) {              // a singular W: the bin goes back to W = I and comes back as X
          st = IVA_BAD_SOLVE;
          if (in) W[bin * (D * D) + r * D + c] = make_double2(r == c ? 1.0 : 0.0, 0.0);
          if (lane == 0) status[bin] = st;
        }
        if (in) Ws[r * D + c] = w;
        if (in && r == ref) As[c] = inv;               // A[ref][c]
      }
      if (lane == 0) s_pass = st;
    }
    __syncthreads();
    const C* xg = (const C*)X + ((long)b * D * F + f) * T;
    C* yg = (C*)Y + ((long)b * D * F + f) * T;
    if (s_pass != 0) {
      for (int t = tid; t < T; t += IVA_THREADS)
#pragma unroll
        for (int d = 0; d < D; ++d) yg[d * chan_stride + t] = xg[d * chan_stride + t];
    } else {
      // up to D = 4 one pass writes the D sources of a frame; above it a pass per source, each holding one row of W (all
      // of W and the D frames' values together are past 256 registers at D = 8); the bin's rows then come from cache
      constexpr int KP = D <= 4 ? D : 1;               // the sources of a pass
      for (int k0 = 0; k0 < D; k0 += KP) {
        double2 wk[KP][D], ak[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          ak[k] = As[k0 + k];
#pragma unroll
          for (int d = 0; d < D; ++d) wk[k][d] = Ws[(k0 + k) * D + d];
        }
        for (int t = tid; t < T; t += IVA_THREADS) {
          C v[D];
#pragma unroll
          for (int d = 0; d < D; ++d) v[d] = xg[d * chan_stride + t];
          double2 x[D];
#pragma unroll
          for (int d = 0; d < D; ++d) x[d] = make_double2((double)v[d].x, (double)v[d].y);
#pragma unroll
          for (int k = 0; k < KP; ++k) {
            double2 y = cmul(wk[k][0], x[0]);
#pragma unroll
            for (int d = 1; d < D; ++d) {
              const double2 q = cmul(wk[k][d], x[d]);
              y.x += q.x;
              y.y += q.y;
            }
            const double2 img = cmul(ak[k], y);
            C out;
            out.x = (R)img.x;
            out.y = (R)img.y;
            yg[(k0 + k) * chan_stride + t] = out;
          }
        }
      }
    }
    __syncthreads();                                   // Ws, As and s_pass are free for the next bin
  }
}

}  // namespace alvq
