// AuxIVA blind source separation of a microphone array's complex spectrograms (auxiliary-function independent vector analysis
// with iterative projection; Ono, WASPAA 2011) and the ratio masks of its output.  The definitions are the comment on
// alvq_auxiva_* / alvq_separation_masks_* in include/alvq.h; tests/helpers/iva_ref.py restates them in numpy.  All arithmetic is
// float64; only Y is rounded.
//
// iva_check_kernel<R>      one pass over X, a wave a (b, f) bin (four bins a workgroup): status 1 for a non-finite value or a bin of
//                     zeros, 0 otherwise, and the start of W: I, or the caller's W0 where the status is 0.
// iva_activity_kernel<R, D>  step 1.  The grid runs over (frame tiles of IVA_TILE = 64, b); a workgroup has D waves, wave k owns
//                     source k and a lane a frame t.  It walks f rising, loads the D values x_d[f, t] (coalesced along t; the
//                     D waves read the same lines) and row k of the bin's W (every lane the same 16 D bytes: scalar loads), and
//                     adds |y_k|^2 to one accumulator; a bin of status 1 is loaded and dropped, so that the loop has no branch
//                     and four bins' loads are in flight.  It stores p (B, D, T) into the workspace.  The order over f is
//                     fixed, so an item has the same bits alone or in a batch, and with or without a bin of status 1.
// iva_weights_kernel  step 2, a workgroup a row (b, k) of p: max_t p by block_max_or (a maximum has no order), then phi over p
//                     in place.
// iva_cov_kernel<R, D>  step 3, the hot loop: X once more.  A wave owns a pair (bin, k), four pairs a workgroup, no LDS and
//                     no barrier; the D waves of a bin are neighbours and read the same X rows from cache, each with its own
//                     phi row.  bf_cov_kernel's per-thread layout: lane l adds the frames t = l, l + 64, ... rising to D^2
//                     float64 accumulators (the lower triangle, the diagonal real), the 64 lane sums meet in wave_sum's
//                     butterfly, each total is divided by T and lane e stores entry e of the full Hermitian matrix (above the
//                     diagonal the exact conjugate) to the workspace: V (B, F, D, D, D).
// iva_solve_kernel<D>  a wave a bin, four bins a workgroup, no LDS and no barrier: the D sequential solves in the lane-per-entry
//                     layout of bf_mvdr_kernel: lane 8 r + c holds entry (r, c) of W, of W V_k and of the right-hand side, and
//                     rows and columns travel by __shfl (iva_solve: Gaussian elimination with partial pivoting, then back
//                     substitution j falling, one subtraction per column on every entry).  Every lane sees the same pivots, so
//                     the status is the same in the whole wave.  v_mfma_f64 is not used, for the reason csrc/wpe.hip gives.
// TWO DIVERGENCES from the suggested plan of 1 + 2 iterations + 1 launches; there are 1 + 4 iterations + 1.
//   The weights have a launch of their own: max_t runs over every frame tile of the item, so a tile's workgroup of
//   iva_activity_kernel cannot know it, and taking it inside the update would repeat a square root and a division per (k, t)
//   in every one of the F bins -- at D = 2 more arithmetic than the covariance itself.
//   The update is two launches, covariances and solves, with V_k passing through 16 D^3 bytes a bin of workspace.  Fused --
//   a workgroup of D waves a bin, V_k in LDS, wave 0 solving behind a barrier -- the D solves are one chain of dependent
//   shuffles and divisions, about 8 D of them each, on one wave while D - 1 wait, and at the 200 registers the D = 8
//   accumulators take a CU holds one such workgroup: measured at (B, D, F, T) = (8, 8, 201, 500), 0.49 ms of a 1.45 ms iteration
//   (0.95 ms were the activity pass, then one wave a frame tile and item for all D sources: 64 waves on the chip).  A wave a bin
//   in a launch of its own (155 registers at D = 8) keeps twelve such chains a CU in flight.  The bits are the same either way.
// iva_project_kernel<R, D>  a workgroup of 256 threads a bin: wave 0 inverts W by iva_solve with D right-hand sides and leaves
//                     W and the row A[ref, :] in LDS; then every thread streams frames t = tid, tid + 256, ...: D loads in
//                     flight, y_k with d rising from the first product, times A[ref, k], rounded and stored.  Up to D = 4 one
//                     pass writes all D sources; above it a pass per source holds one row of W in registers (all of W next to a
//                     frame's D values took 256 VGPRs and 104 AGPRs at D = 8: one wave a SIMD) and rereads the bin's rows,
//                     16 D T bytes, from cache.  A bin whose status is not 0 is copied, bit for bit.
// iva_masks_kernel<R, K>   elementwise, a thread a (b, f, t).
// Every grid but iva_activity_kernel's (at most 1024 x 65535) and iva_weights_kernel's (B D <= 524 280) is capped at
// IVA_MAX_BLOCKS workgroups and strides over the bins (pairs, outputs) beyond, whole waves or whole workgroups at a time.
// No atomics anywhere, no host-side decision between the launches: the status is read on the device.
// What the launches cost: DESIGN.md.
#include <cfloat>
#include <climits>
#include <cmath>

#include "alvq_common.h"

namespace alvq {

constexpr int IVA_THREADS = 256;
constexpr int IVA_WAVES = IVA_THREADS / kWave;
constexpr int IVA_TILE = 64;               // the frames of a workgroup of iva_activity_kernel: a lane each, in every wave
constexpr int IVA_MAX_D = 8;
constexpr int IVA_MAX_T = 65535;
constexpr int IVA_MAX_ITERATIONS = 256;
constexpr long IVA_MAX_BLOCKS = 1 << 16;

constexpr int IVA_BAD_INPUT = 1;           // a non-finite value in the bin, or a bin of zeros
constexpr int IVA_BAD_SOLVE = 2;           // a pivot or Re(w^H V w) that is 0 (<= 0) or not finite, or a singular W at the end

constexpr int IVA_LAPLACE = 0, IVA_GAUSS = 1;

template <typename R> struct IvaCplx;
template <> struct IvaCplx<float> { typedef float2 type; };
template <> struct IvaCplx<double> { typedef double2 type; };

__device__ __forceinline__ bool iva_finite(double v) { return fabs(v) <= DBL_MAX; }

__device__ __forceinline__ double2 iva_mul(double2 a, double2 b) {           // a b
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 iva_div(double2 a, double2 p) {           // a / p as a conj(p) / |p|^2
  const double den = p.x * p.x + p.y * p.y;
  return make_double2((a.x * p.x + a.y * p.y) / den, (a.y * p.x - a.x * p.y) / den);
}
__device__ __forceinline__ double2 iva_shfl(double2 v, int src) {
  return make_double2(__shfl(v.x, src, 64), __shfl(v.y, src, 64));
}

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
    m = iva_shfl(m, 8 * src + c);
    rhs = iva_shfl(rhs, 8 * src + c);
    const double2 piv = iva_shfl(m, 9 * j), mrj = iva_shfl(m, 8 * r + j), mjc = iva_shfl(m, 8 * j + c);
    const double2 bjc = iva_shfl(rhs, 8 * j + c);
    if (r > j) {
      const double2 l = iva_div(mrj, piv);
      const double2 pm = iva_mul(l, mjc), pb = iva_mul(l, bjc);
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
    const double2 piv = iva_shfl(m, 9 * j), bjc = iva_shfl(rhs, 8 * j + c), mrj = iva_shfl(m, 8 * r + j);
    const double2 z = iva_div(bjc, piv);
    if (r == j) {
      rhs = z;
    } else if (r < j) {
      const double2 pz = iva_mul(mrj, z);
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
  typedef typename IvaCplx<R>::type C;
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
        if (!iva_finite(re) || !iva_finite(im)) bad = 1;
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

// ----------------------------------------------------------------------------------------------------------------- activity
template <typename R, int D>
__global__ __launch_bounds__(kWave * D) void iva_activity_kernel(const void* X, const double2* W, const int* status, double* P, int F,
                                                                int T) {
  typedef typename IvaCplx<R>::type C;
  const int lane = threadIdx.x & 63;
  const int k = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));          // wave k of the workgroup owns source k
  const int b = blockIdx.y, t = blockIdx.x * IVA_TILE + lane;
  const bool live = t < T;
  const long chan_stride = (long)F * T;
  const C* xg = (const C*)X + (long)b * D * chan_stride + (live ? t : T - 1);      // a lane past the row reads its last frame
  double p = 0.0;
#pragma unroll 4
  for (int f = 0; f < F; ++f) {
    const long bin = (long)b * F + f;
    const bool skip = status[bin] == IVA_BAD_INPUT;    // the same in every lane; what the bin holds is loaded and dropped
    const double2* w = W + bin * (D * D) + k * D;
    double2 x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const C v = xg[d * chan_stride + (long)f * T];
      x[d] = make_double2((double)v.x, (double)v.y);
    }
    double2 y = iva_mul(w[0], x[0]);
#pragma unroll
    for (int d = 1; d < D; ++d) {
      const double2 q = iva_mul(w[d], x[d]);
      y.x += q.x;
      y.y += q.y;
    }
    const double q = fma(y.y, y.y, fma(y.x, y.x, p));
    p = skip ? p : q;
  }
  if (live) P[((long)b * D + k) * T + t] = p;
}

// ------------------------------------------------------------------------------------------------------------------ weights
__global__ __launch_bounds__(IVA_THREADS) void iva_weights_kernel(double* P, int F, int T, int model, double eps) {
  __shared__ double s_max[IVA_WAVES];
  __shared__ int s_flag[IVA_WAVES];
  const int tid = threadIdx.x;
  double* row = P + (long)blockIdx.x * T;
  double top = 0.0;
  int bad = 0;
  for (int t = tid; t < T; t += IVA_THREADS) {
    const double v = row[t];                           // a sum of squares: >= 0, or not finite
    if (!(v <= DBL_MAX)) bad = 1;
    else top = fmax(top, v);
  }
  block_max_or<false>(top, bad, s_max, s_flag);
  const bool flat = bad || !(top > 0.0);               // max_t is 0 or not finite: phi = 1
  const double low = model == IVA_LAPLACE ? eps * sqrt(top) : eps * top;
  for (int t = tid; t < T; t += IVA_THREADS) {         // a thread rewrites what it read itself
    const double v = row[t];
    double phi = 1.0;
    if (!flat) phi = model == IVA_LAPLACE ? 1.0 / fmax(sqrt(v), low) : (double)F / fmax(v, low);
    row[t] = phi;
  }
}

// --------------------------------------------------------------------------------------------------------------- covariance
template <typename R, int D>
__global__ __launch_bounds__(IVA_THREADS) void iva_cov_kernel(const void* X, const double* Phi, const int* status, double2* V,
                                                              long nbins, int F, int T) {
  typedef typename IvaCplx<R>::type C;
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
    const double* phi = Phi + ((long)b * D + k) * T;

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
template <int D>
__global__ __launch_bounds__(IVA_THREADS) void iva_solve_kernel(const double2* Vg, double2* W, int* status, long nbins) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane >> 3, c = lane & 7;
  const bool in = r < D && c < D;
  const int at = in ? r * D + c : 0;                   // a lane outside the block loads entry 0 and drops it
  const double2 zero = make_double2(0.0, 0.0);
  // the grid is capped: a wave strides over its bins, whole, and meets no barrier anywhere
  for (long bin = (long)blockIdx.x * IVA_WAVES + wv; bin < nbins; bin += (long)gridDim.x * IVA_WAVES) {
    if (status[bin] != 0) continue;
    double2 w = W[bin * (D * D) + at];
    if (!in) w = zero;
    int fail = 0;
    for (int k = 0; k < D && !fail; ++k) {             // `fail` is the same in every lane
      const double2* V = Vg + (bin * D + k) * (D * D);
      double2 m = zero;                                // (W V_k)[r][c], j rising from the first product
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 wrj = iva_shfl(w, 8 * r + j);
        const double2 q = iva_mul(wrj, V[in ? j * D + c : 0]);
        m = j == 0 ? q : make_double2(m.x + q.x, m.y + q.y);
      }
      if (!in) m = zero;
      double2 sol = make_double2(r == k ? 1.0 : 0.0, 0.0);            // e_k in every column
      fail = iva_solve<D>(m, sol, r, c);               // the lanes of row r hold w_r
      const double2 wc = iva_shfl(sol, 8 * c);
      const double2 term = in ? iva_mul(V[at], wc) : zero;
      double2 vw = zero;                               // (V_k w)[r], c rising from the first product
#pragma unroll
      for (int cc = 0; cc < D; ++cc) {
        const double2 q = iva_shfl(term, 8 * r + cc);
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
  typedef typename IvaCplx<R>::type C;
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
            double2 y = iva_mul(wk[k][0], x[0]);
#pragma unroll
            for (int d = 1; d < D; ++d) {
              const double2 q = iva_mul(wk[k][d], x[d]);
              y.x += q.x;
              y.y += q.y;
            }
            const double2 img = iva_mul(ak[k], y);
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

// -------------------------------------------------------------------------------------------------------------------- masks
template <typename R, int K>
__global__ __launch_bounds__(IVA_THREADS) void iva_masks_kernel(const void* Y, double* M, long nbins, int F, int T) {
  typedef typename IvaCplx<R>::type C;
  const long total = nbins * T, chan_stride = (long)F * T;
  for (long e = (long)blockIdx.x * IVA_THREADS + threadIdx.x; e < total; e += (long)gridDim.x * IVA_THREADS) {
    const long bin = e / T;
    const int t = (int)(e - bin * T);
    const int b = (int)(bin / F), f = (int)(bin % F);
    const long at = ((long)b * K * F + f) * T + t;
    double q[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const C v = ((const C*)Y)[at + k * chan_stride];
      const double re = (double)v.x, im = (double)v.y;
      q[k] = re * re + im * im;
    }
    double s = q[0];
#pragma unroll
    for (int k = 1; k < K; ++k) s += q[k];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double m = 0.0;                                  // a sum that is not finite
      if (s == 0.0) m = 1.0 / (double)K;
      else if (iva_finite(s)) m = q[k] / s;
      M[at + k * chan_stride] = m;
    }
  }
}

}  // namespace alvq

using namespace alvq;

static dim3 iva_grid(long blocks) { return dim3((unsigned)(blocks < IVA_MAX_BLOCKS ? blocks : IVA_MAX_BLOCKS)); }

static int iva_check_dims(const char* who, int B, int D, int F, int T) {
  ALVQ_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && (long)B * F <= INT_MAX, ALVQ_EINVAL,
               "%s: B=%d F=%d (need 1 <= B <= 65535, F >= 1, B F <= 2^31 - 1)", who, B, F);
  ALVQ_REQUIRE(D >= 1 && D <= IVA_MAX_D, ALVQ_EINVAL, "%s: D=%d (need 1 <= D <= 8)", who, D);
  ALVQ_REQUIRE(T >= 1 && T <= IVA_MAX_T, ALVQ_EINVAL, "%s: T=%d (need 1 <= T <= 65535)", who, T);
  return ALVQ_OK;
}

#define IVA_FOR_D(D, CALL)  \
  switch (D) {              \
    case 1: CALL(1); break; \
    case 2: CALL(2); break; \
    case 3: CALL(3); break; \
    case 4: CALL(4); break; \
    case 5: CALL(5); break; \
    case 6: CALL(6); break; \
    case 7: CALL(7); break; \
    default: CALL(8); break; \
  }

static int64_t iva_phi_bytes(int B, int D, int T) { return ((int64_t)8 * B * D * T + 15) / 16 * 16; }

extern "C" int64_t alvq_auxiva_workspace_bytes(int B, int D, int F, int T) {
  if (B < 1 || B > 65535 || F < 1 || (long)B * F > INT_MAX || D < 1 || D > IVA_MAX_D || T < 1 || T > IVA_MAX_T) return -1;
  // p, then phi over it: (B, D, T) float64; the D weighted covariances of every bin: (B, F, D, D, D) complex128
  return iva_phi_bytes(B, D, T) + (int64_t)16 * B * F * D * D * D;
}

template <typename R>
static int iva_launch(const char* who, const R* X, const double* W0, double* W, R* Y, int* status, void* workspace, int B, int D, int F,
                      int T, int model, int iterations, int ref, double eps, void* stream) {
  ALVQ_REQUIRE(X && W && Y && status && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  const int rc = iva_check_dims(who, B, D, F, T);
  if (rc != ALVQ_OK) return rc;
  ALVQ_REQUIRE(model == IVA_LAPLACE || model == IVA_GAUSS, ALVQ_EINVAL, "%s: model=%d (need 0 = laplace or 1 = gauss)", who, model);
  ALVQ_REQUIRE(iterations >= 0 && iterations <= IVA_MAX_ITERATIONS, ALVQ_EINVAL, "%s: iterations=%d (need 0 <= iterations <= 256)", who,
               iterations);
  ALVQ_REQUIRE(ref >= 0 && ref < D, ALVQ_EINVAL, "%s: ref=%d (need 0 <= ref < D = %d)", who, ref, D);
  ALVQ_REQUIRE(std::isfinite(eps) && eps >= 0.0, ALVQ_EINVAL, "%s: eps=%g must be finite and >= 0", who, eps);
  const long nbins = (long)B * F;
  hipStream_t s = (hipStream_t)stream;
  double* P = (double*)workspace;
  double2* Wd = (double2*)W;
  hipLaunchKernelGGL((iva_check_kernel<R>), iva_grid((nbins + IVA_WAVES - 1) / IVA_WAVES), dim3(IVA_THREADS), 0, s, (const void*)X,
                     (const double2*)W0, Wd, status, nbins, D, F, T);
  double2* V = (double2*)((char*)workspace + iva_phi_bytes(B, D, T));
  const dim3 tiles((unsigned)((T + IVA_TILE - 1) / IVA_TILE), (unsigned)B);
  const dim3 cov_grid = iva_grid((nbins * D + IVA_WAVES - 1) / IVA_WAVES), solve_grid = iva_grid((nbins + IVA_WAVES - 1) / IVA_WAVES);
  for (int it = 0; it < iterations; ++it) {
#define IVA_CALL(N) \
  hipLaunchKernelGGL((iva_activity_kernel<R, N>), tiles, dim3(kWave * N), 0, s, (const void*)X, (const double2*)Wd, (const int*)status, P, F, T)
    IVA_FOR_D(D, IVA_CALL)
#undef IVA_CALL
    hipLaunchKernelGGL(iva_weights_kernel, dim3((unsigned)(B * D)), dim3(IVA_THREADS), 0, s, P, F, T, model, eps);
#define IVA_CALL(N) \
  hipLaunchKernelGGL((iva_cov_kernel<R, N>), cov_grid, dim3(IVA_THREADS), 0, s, (const void*)X, (const double*)P, (const int*)status, V, nbins, F, T)
    IVA_FOR_D(D, IVA_CALL)
#undef IVA_CALL
#define IVA_CALL(N) hipLaunchKernelGGL((iva_solve_kernel<N>), solve_grid, dim3(IVA_THREADS), 0, s, (const double2*)V, Wd, status, nbins)
    IVA_FOR_D(D, IVA_CALL)
#undef IVA_CALL
  }
#define IVA_CALL(N) \
  hipLaunchKernelGGL((iva_project_kernel<R, N>), iva_grid(nbins), dim3(IVA_THREADS), 0, s, (const void*)X, Wd, (void*)Y, status, nbins, F, T, ref)
  IVA_FOR_D(D, IVA_CALL)
#undef IVA_CALL
  return check_launch(who);
}

extern "C" int alvq_auxiva_f32(const float* X, const double* W0, double* W, float* Y, int* status, void* workspace, int B, int D,
                               int F, int T, int model, int iterations, int ref, double eps, void* stream) {
  return iva_launch("alvq_auxiva_f32", X, W0, W, Y, status, workspace, B, D, F, T, model, iterations, ref, eps, stream);
}

extern "C" int alvq_auxiva_f64(const double* X, const double* W0, double* W, double* Y, int* status, void* workspace, int B, int D,
                               int F, int T, int model, int iterations, int ref, double eps, void* stream) {
  return iva_launch("alvq_auxiva_f64", X, W0, W, Y, status, workspace, B, D, F, T, model, iterations, ref, eps, stream);
}

template <typename R>
static int iva_masks_launch(const char* who, const R* Y, double* M, int B, int K, int F, int T, void* stream) {
  ALVQ_REQUIRE(Y && M, ALVQ_EINVAL, "%s: null pointer", who);
  const int rc = iva_check_dims(who, B, K, F, T);
  if (rc != ALVQ_OK) return rc;
  const long nbins = (long)B * F;
  const dim3 grid = iva_grid((nbins * T + IVA_THREADS - 1) / IVA_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define IVA_CALL(N) hipLaunchKernelGGL((iva_masks_kernel<R, N>), grid, dim3(IVA_THREADS), 0, s, (const void*)Y, M, nbins, F, T)
  IVA_FOR_D(K, IVA_CALL)
#undef IVA_CALL
  return check_launch(who);
}

extern "C" int alvq_separation_masks_f32(const float* Y, double* M, int B, int K, int F, int T, void* stream) {
  return iva_masks_launch("alvq_separation_masks_f32", Y, M, B, K, F, T, stream);
}

extern "C" int alvq_separation_masks_f64(const double* Y, double* M, int B, int K, int F, int T, void* stream) {
  return iva_masks_launch("alvq_separation_masks_f64", Y, M, B, K, F, T, stream);
}
