// Beamforming of a microphone array's complex spectrograms: spatial covariances, steering vectors, delay-and-sum / MVDR weights
// (with a steering vector, or from two covariances after Souden, Benesty, Affes 2010) and their application.  The definitions
// are the comment on alvq_spatial_covariance_* / alvq_steering_vectors_f64 / alvq_beamform_weights_f64 / alvq_beamform_apply_*
// in include/alvq.h; tests/helpers/beamform_ref.py restates them in numpy.  All arithmetic is float64; only Y is rounded.
//
// bf_cov_kernel<R, D, W>  the hot loop: the whole spectrogram once.  W waves own a (b, f) bin: W = 1 where T <= BF_WAVE_T = 1024
//                    (a 256-thread workgroup then holds four bins, a wave each, and passes no barrier), W = 4 above it (the
//                    workgroup owns the bin).  A thread loads frame t of the bin's D rows (D loads in flight, coalesced along
//                    t), and adds (m_t x_i) conj(x_j), i >= j, by fused multiply-adds to D^2 float64
//                    accumulators and m_t to one more, all in registers (D is a template argument: the loops are unrolled;
//                    the diagonal has no imaginary accumulator, so it is exactly 0).  Sum order: a thread takes
//                    t = l, l + 64 W, ... rising (l its lane, or its thread index where W = 4), the 64 lane sums meet in
//                    wave_sum's butterfly, and where W = 4 the four wave totals are added kSequential.  W depends on T alone, so
//                    the order depends on (D, T) alone.  Every lane ends with every total; lane e < D^2 picks entry e
//                    (the upper triangle as the negated imaginary part of the lower) and divides it by the mask's sum: one
//                    coalesced store of the bin's matrix.
// bf_steer_kernel    a workgroup an item, a thread an entry (d, f): two distances (csrc/steered_map.h's steer_delay), one
//                    sincospi on tau_d - tau_ref.  A non-finite coordinate sets that header's geometry bit.
// bf_das_kernel      w = a / D, a thread an entry.
// bf_mvdr_kernel     a wave a bin, four bins a workgroup, no LDS and no barrier: lane 8 r + c holds entry (r, c) of the
//                    loaded Phi_n and of the right-hand sides (column 0 = a, or the D columns of Phi_s), and rows and columns
//                    travel by __shfl.  Right-looking Cholesky on the lower triangle (column k = 0 .. D - 1: the pivot's
//                    square root divides the column, then one subtraction on every entry below and right of it), forward
//                    substitution k rising, back substitution k falling, one subtraction per column on every entry: WPE's
//                    order.  tr Phi_n, Re(a^H z) and Re tr G are added from 0 with the index rising.  The problem is 8 x 8 at
//                    most, so v_mfma_f64 is not used, for the reason csrc/wpe.hip gives: it buys no arithmetic at the float64
//                    vector rate and would bring a sum order of its own.
// bf_gev_kernel      the same layout, factorisation and substitutions (bf_cholesky, bf_forward, bf_backward serve both
//                    kernels): Y = L^-1 Phi_s, then L^-1 Y^H after a conjugate transposition by one shuffle, whose lower
//                    triangle is C = L^-1 Phi_s L^-H; csrc/herm_eig.h takes its eigendecomposition in place; the top
//                    eigenvector u goes back through L^H (v) and forward through L (a, k rising from the first term).
// bf_apply_kernel<R, D>  one streaming pass: a thread an output (b, f, t) of the flattened B F T outputs, so that a row
//                    shorter than the workgroup leaves no thread idle; it holds the bin's D weights in registers (lanes of a
//                    wave read the same 16 D bytes: one cache line or two), has its D loads of X in flight together, and
//                    adds conj(w_d) x_d[t] with d rising, starting from the first product.  A weight of exactly 0 is passed
//                    over and a weight with an imaginary part of exactly 0 multiplies as a real number, so that w = e_ref
//                    returns x_ref bit for bit whatever the bin holds, a NaN included.
// Every grid is capped at kMaxBlocks workgroups and strides over the bins (or outputs) beyond, whole waves or whole
// workgroups at a time.  No atomics anywhere; a bin shares nothing with its neighbours: it has the same bits alone, in any
// batch and on any run.
// What the launches cost: DESIGN.md.
#include "herm_eig.h"
#include "steered_map.h"

namespace alvq {

constexpr int BF_THREADS = 256;
constexpr int BF_WAVES = BF_THREADS / kWave;
constexpr int BF_WAVE_T = 1024;        // rows up to this long are summed by one wave, longer ones by the workgroup

// status values of alvq_spatial_covariance_* and alvq_beamform_weights_f64
constexpr int BF_BAD_INPUT = 1;        // a non-finite X, a negative or non-finite mask value, or a mask that sums to 0
constexpr int BF_BAD_SOLVE = 2;        // a Cholesky pivot or the denominator <= 0 or not finite

constexpr int BF_DAS = 0, BF_MVDR = 1, BF_SOUDEN = 2;

// ------------------------------------------------------------------------------------------------------- spatial covariance
struct BfCovArgs {
  const void* X;
  const double* mask;
  double2* Phi;
  int* status;
  long nbins;
  int F, T;
};

template <typename R, int D, int W>
__global__ __launch_bounds__(BF_THREADS, 2) void bf_cov_kernel(BfCovArgs a) {   // two waves a SIMD: 256 registers
  typedef typename Cplx<R>::type C;
  constexpr int K = D * D + 1;                       // D real diagonal sums, D (D - 1) / 2 complex ones below it, the mask's sum
  __shared__ double red[W == 1 ? 1 : K][BF_WAVES];
  __shared__ int s_flag[BF_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = a.T;
  // the grid is capped: a wave (W = 1) or the workgroup strides over its bins; where W = 4 every thread of the workgroup
  // makes the same passes, so the barriers are met
  const long first = W == 1 ? (long)blockIdx.x * BF_WAVES + wv : (long)blockIdx.x;
  const long stride = W == 1 ? (long)gridDim.x * BF_WAVES : (long)gridDim.x;
  for (long bin = first; bin < a.nbins; bin += stride) {
  const int b = (int)(bin / a.F), f = (int)(bin % a.F);
  const long chan_stride = (long)a.F * T;
  const C* Xg = (const C*)a.X + ((long)b * D * a.F + f) * T;
  const double* mg = a.mask ? a.mask + bin * T : nullptr;

  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  int bad = 0;
  // one frame into the accumulators: y = m x_i first, then re += y.re x_j.re, re += y.im x_j.im and im += y.im x_j.re,
  // im -= y.re x_j.im as fused multiply-adds, in that order; on the diagonal the real part alone
  auto add_frame = [&](const C(&v)[D], double m) {
    if (!(m >= 0.0 && m <= DBL_MAX)) bad = 1;
    double2 x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      x[d] = make_double2((double)v[d].x, (double)v[d].y);
      if (!is_finite(x[d].x) || !is_finite(x[d].y)) bad = 1;
    }
    int k = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double2 y = make_double2(m * x[i].x, m * x[i].y);
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        acc[k] = fma(y.y, x[j].y, fma(y.x, x[j].x, acc[k]));
        ++k;
        if (j < i) {
          acc[k] = fma(-y.x, x[j].y, fma(y.y, x[j].x, acc[k]));
          ++k;
        }
      }
    }
    acc[K - 1] += m;
  };
  for (int t = W == 1 ? lane : tid; t < T; t += W * kWave) {
    C v[D];
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = Xg[d * chan_stride + t];
    add_frame(v, mg ? mg[t] : 1.0);
  }

  if constexpr (W == 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = wave_sum(acc[k]);
    bad = wave_or(bad);
  } else {
    bad = wave_or(bad);
    if (lane == 0) s_flag[wv] = bad;                 // read after block_sum's barrier
    block_sum<kSequential, false>(acc, red);
    bad = s_flag[0] | s_flag[1] | s_flag[2] | s_flag[3];
  }
  const double ms = acc[K - 1];
  const int fail = (bad || !(ms > 0.0)) ? BF_BAD_INPUT : 0;

  if (W == 1 || wv == 0) {
  double re = 0.0, im = 0.0;                         // lane e = i D + j picks its entry; the divisions come after the choice
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const double sr = acc[k++];
        const double si = j < i ? acc[k++] : 0.0;
        if (lane == i * D + j) {
          re = sr;
          im = si;
        }
        if (j < i && lane == j * D + i) {
          re = sr;
          im = -si;                                  // the exact conjugate: a division keeps the sign
        }
      }
  }
  if (lane < D * D) {
    double2 out = make_double2(0.0, 0.0);
    if (!fail) {
      out.x = re / ms;
      out.y = (lane / D == lane % D) ? 0.0 : im / ms;
    }
    a.Phi[bin * (D * D) + lane] = out;
  }
  if (lane == 0) a.status[bin] = fail;
  }
  if (W != 1) __syncthreads();                       // red and s_flag are free for the next bin
  }
}

// --------------------------------------------------------------------------------------------------------- steering vectors
__global__ __launch_bounds__(BF_THREADS) void bf_steer_kernel(const double* mics, const double* src, double2* A, int* status, int D,
                                                               int F, long mics_stride, double fs_over_n, double c, int ref) {
  const int tid = threadIdx.x, b = blockIdx.x;
  const double* m = mics + (long)b * mics_stride;
  const double* q = src + 3L * b;
  int bad = 0;                                       // the same in every thread
  for (int e = 0; e < 3 * D; ++e)
    if (!is_finite(m[e])) bad = 1;
  const double qx = q[0], qy = q[1], qz = q[2];
  if (!is_finite(qx) || !is_finite(qy) || !is_finite(qz)) bad = 1;
  const double tau_ref = steer_delay(qx, qy, qz, m, ref, c);
  double2* out = A + (long)b * D * F;
  for (int e = tid; e < D * F; e += BF_THREADS) {
    const int d = e / F, f = e - d * F;
    double2 v = make_double2(__longlong_as_double(0x7ff8000000000000LL), __longlong_as_double(0x7ff8000000000000LL));
    if (!bad) {
      double s, cs;
      sincospi((double)(2 * f) * fs_over_n * (steer_delay(qx, qy, qz, m, d, c) - tau_ref), &s, &cs);      // e^{-j pi x}
      v = make_double2(cs, -s);
    }
    out[e] = v;
  }
  if (tid == 0) status[b] = bad ? MAP_BAD_GEOMETRY : 0;
}

// ------------------------------------------------------------------------------------------------------------------ weights
struct BfWeightArgs {
  const double2* Phi_n;
  const double2* Phi_s;
  const double2* A;
  double2* W;
  int* status;
  long nbins;
  int D, F, mode, ref;
  double loading;
};

__global__ __launch_bounds__(BF_THREADS) void bf_das_kernel(BfWeightArgs a) {
  for (long e = (long)blockIdx.x * BF_THREADS + threadIdx.x; e < a.nbins * a.D; e += (long)gridDim.x * BF_THREADS) {      // (bin, d)
    const long bin = e / a.D;
    const int d = (int)(e - bin * a.D);
    const int b = (int)(bin / a.F), f = (int)(bin % a.F);
    const double2 v = a.A[((long)b * a.D + d) * a.F + f];
    a.W[e] = make_double2(v.x / (double)a.D, v.y / (double)a.D);
    if (d == 0) a.status[bin] = 0;
  }
}

// The factorisation and the two substitutions of bf_mvdr_kernel and bf_gev_kernel, on the wave's layout: lane 8 r + c holds
// entry (r, c) of the matrix and entry r of right-hand side c.  Right-looking Cholesky on the lower triangle: column k of L
// replaces column k of m, the pivot stays on the diagonal.  BF_BAD_SOLVE where a pivot is <= 0 or not finite.
__device__ __forceinline__ int bf_cholesky(double2& m, int D, int r, int c, bool in) {
  int fail = 0;
  for (int k = 0; k < D; ++k) {
    const double piv = __shfl(m.x, 9 * k, 64);
    if (!(piv > 0.0 && piv <= DBL_MAX)) fail = BF_BAD_SOLVE;
    const double l = sqrt(piv);
    if (in && c == k && r > k) {
      m.x /= l;
      m.y /= l;
    }
    const double2 lr = cshfl(m, 8 * r + k), lc = cshfl(m, 8 * c + k);
    if (in && c > k && r >= c) {
      const double2 p = cmul_conj(lr, lc);
      m.x -= p.x;
      m.y -= p.y;
    }
  }
  return fail;
}

__device__ __forceinline__ void bf_forward(const double2& m, double2& rhs, int D, int r, int c, bool in) {      // L y = rhs
  for (int k = 0; k < D; ++k) {
    const double l = sqrt(__shfl(m.x, 9 * k, 64));
    if (r == k) {
      rhs.x /= l;
      rhs.y /= l;
    }
    const double2 yk = cshfl(rhs, 8 * k + c), lrk = cshfl(m, 8 * r + k);
    if (in && r > k) {
      const double2 p = cmul(lrk, yk);
      rhs.x -= p.x;
      rhs.y -= p.y;
    }
  }
}

__device__ __forceinline__ void bf_backward(const double2& m, double2& rhs, int D, int r, int c) {             // L^H z = y
  for (int k = D - 1; k >= 0; --k) {
    const double l = sqrt(__shfl(m.x, 9 * k, 64));
    if (r == k) {
      rhs.x /= l;
      rhs.y /= l;
    }
    const double2 zk = cshfl(rhs, 8 * k + c), lkr = cshfl(m, 8 * k + r);
    if (r < k) {
      const double2 p = conj_cmul(lkr, zk);
      rhs.x -= p.x;
      rhs.y -= p.y;
    }
  }
}

__global__ __launch_bounds__(BF_THREADS) void bf_mvdr_kernel(BfWeightArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int D = a.D, r = lane >> 3, c = lane & 7;
  const bool in = r < D && c < D;
  // the grid is capped: a wave strides over its bins, whole, and meets no barrier anywhere
  for (long bin = (long)blockIdx.x * BF_WAVES + wv; bin < a.nbins; bin += (long)gridDim.x * BF_WAVES) {
  const int b = (int)(bin / a.F), f = (int)(bin % a.F);
  const double2 zero = make_double2(0.0, 0.0);

  double2 m = in ? a.Phi_n[bin * (D * D) + r * D + c] : zero;              // entry (r, c); only r >= c is ever used
  double2 rhs = zero;                                                      // entry r of right-hand side c
  if (a.mode == BF_MVDR) {
    if (r < D && c == 0) rhs = a.A[((long)b * D + r) * a.F + f];
  } else if (in) {
    rhs = a.Phi_s[bin * (D * D) + r * D + c];
  }
  const double2 steer = rhs;

  double tr = 0.0;
  for (int i = 0; i < D; ++i) tr += __shfl(m.x, 9 * i, 64);
  const double load = a.loading * (tr / (double)D);
  if (in && r == c) m.x += load;

  // every lane sees the same pivots and the same denominator, so `fail` is the same in the whole wave
  int fail = bf_cholesky(m, D, r, c, in);
  bf_forward(m, rhs, D, r, c, in);                   // L y = rhs
  bf_backward(m, rhs, D, r, c);                      // L^H z = y

  double den = 0.0;
  if (a.mode == BF_MVDR) {
    const double term = steer.x * rhs.x + steer.y * rhs.y;                 // Re(conj(a_r) z_r) in the lanes (r, 0)
    for (int i = 0; i < D; ++i) den += __shfl(term, 8 * i, 64);
  } else {
    for (int i = 0; i < D; ++i) den += __shfl(rhs.x, 9 * i, 64);          // Re tr G
  }
  if (!(den > 0.0 && den <= DBL_MAX)) fail = BF_BAD_SOLVE;

  const int col = a.mode == BF_MVDR ? 0 : a.ref;
  if (r < D && c == col) {
    double2 w = make_double2(rhs.x / den, rhs.y / den);
    if (fail) w = make_double2(r == a.ref ? 1.0 : 0.0, 0.0);
    a.W[bin * D + r] = w;
  }
  if (lane == 0) a.status[bin] = fail;
  }
}

// ---------------------------------------------------------------------------------------------------------------------- GEV
struct BfGevArgs {
  const double2* Phi_n;
  const double2* Phi_s;
  double2* W;
  double2* RTF;
  double* gain;
  int* status;
  long nbins;
  int D, ref;
  double loading;
};

__global__ __launch_bounds__(BF_THREADS) void bf_gev_kernel(BfGevArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int D = a.D, r = lane >> 3, c = lane & 7;
  const bool in = r < D && c < D;
  for (long bin = (long)blockIdx.x * BF_WAVES + wv; bin < a.nbins; bin += (long)gridDim.x * BF_WAVES) {
  const double2 zero = make_double2(0.0, 0.0);
  double2 m = in ? a.Phi_n[bin * (D * D) + r * D + c] : zero;
  double2 rhs = in ? a.Phi_s[bin * (D * D) + r * D + c] : zero;

  double tr = 0.0;
  for (int i = 0; i < D; ++i) tr += __shfl(m.x, 9 * i, 64);
  const double load = a.loading * (tr / (double)D);
  if (in && r == c) m.x += load;

  // every lane sees the same pivots, eigenvalues and a_ref, so `fail` is the same in the whole wave
  int fail = bf_cholesky(m, D, r, c, in);
  bf_forward(m, rhs, D, r, c, in);                   // Y = L^-1 Phi_s
  const double2 yt = cshfl(rhs, 8 * c + r);
  rhs = in ? make_double2(yt.x, -yt.y) : zero;       // Y^H
  bf_forward(m, rhs, D, r, c, in);                   // L^-1 Y^H = C: Hermitian but for rounding; its lower triangle counts
  const double2 low = cshfl(rhs, 8 * c + r);
  double2 cm = zero;
  if (in) cm = r > c ? rhs : (r == c ? make_double2(rhs.x, 0.0) : make_double2(low.x, -low.y));

  double2 v;
  const HermEig e = herm_eig(cm, v, D, lane);
  if (e.status) fail = BF_BAD_SOLVE;
  const unsigned long long tops = __ballot(r == 0 && c < D && e.rank == D - 1);
  const int top = tops ? __ffsll((long long)tops) - 1 : 0;                 // the column of the largest eigenvalue
  const double lmax = __shfl(e.lam, top, 64);
  if (!(lmax > 0.0 && lmax <= DBL_MAX)) fail = BF_BAD_SOLVE;

  // a = L u, k rising from the first term; the diagonal of L is the pivot's square root
  double2 av = zero;
  for (int k = 0; k < D; ++k) {
    const double l = sqrt(__shfl(m.x, 9 * k, 64));
    const double2 lrk = cshfl(m, 8 * r + k), uk = cshfl(v, 8 * k + top);
    if (k <= r) {
      const double2 p = k < r ? cmul(lrk, uk) : make_double2(l * uk.x, l * uk.y);
      av = k == 0 ? p : make_double2(av.x + p.x, av.y + p.y);
    }
  }
  const double2 u = cshfl(v, 8 * r + top);
  rhs = (r < D && c == 0) ? u : zero;
  bf_backward(m, rhs, D, r, c);                      // v = L^-H u in the lanes (r, 0)

  const double2 aref = cshfl(av, 8 * a.ref);
  const double den = aref.x * aref.x + aref.y * aref.y;
  if (!(den > 0.0 && den <= DBL_MAX)) fail = BF_BAD_SOLVE;

  if (r < D && c == 0) {
    const double2 num = cmul_conj(av, aref);
    double2 rtf = make_double2(num.x / den, num.y / den);
    double2 w = cmul_conj(rhs, aref);
    if (D == 1) w = rtf = make_double2(1.0, 0.0);
    if (fail) w = rtf = make_double2(r == a.ref ? 1.0 : 0.0, 0.0);
    a.W[bin * D + r] = w;
    a.RTF[bin * D + r] = rtf;
  }
  if (lane == 0) {
    a.gain[bin] = fail ? 0.0 : lmax;
    a.status[bin] = fail;
  }
  }
}

// -------------------------------------------------------------------------------------------------------------------- apply
template <typename R, int D>
__global__ __launch_bounds__(BF_THREADS) void bf_apply_kernel(const void* X, const double2* Wt, void* Y, long nbins, int F, int T) {
  typedef typename Cplx<R>::type C;
  const long total = nbins * T, chan_stride = (long)F * T;
  for (long e0 = (long)blockIdx.x * BF_THREADS; e0 < total; e0 += (long)gridDim.x * BF_THREADS) {
    const long bin0 = e0 / T;                        // the same in the whole workgroup
    const int off = (int)(e0 - bin0 * T) + (int)threadIdx.x;
    const long bin = bin0 + off / T;
    const int t = off % T;
    if (bin >= nbins) continue;
    const int b = (int)(bin / F), f = (int)(bin % F);
    const C* xg = (const C*)X + ((long)b * D * F + f) * T + t;
    const double2* wg = Wt + bin * D;
    C v[D];
    double2 w[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      v[d] = xg[d * chan_stride];
      w[d] = wg[d];
    }
    double2 y = make_double2(0.0, 0.0);
    bool started = false;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (w[d].x == 0.0 && w[d].y == 0.0) continue;   // a weight of exactly 0 adds nothing, whatever its x holds
      const double2 x = make_double2((double)v[d].x, (double)v[d].y);
      const double2 p = w[d].y == 0.0 ? make_double2(w[d].x * x.x, w[d].x * x.y) : conj_cmul(w[d], x);
      y = started ? make_double2(y.x + p.x, y.y + p.y) : p;
      started = true;
    }
    C out;
    out.x = (R)y.x;
    out.y = (R)y.y;
    ((C*)Y)[bin * T + t] = out;
  }
}

}  // namespace alvq

using namespace alvq;

template <typename R>
static int bf_cov_launch(const char* who, const R* X, const double* mask, double* Phi, int* status, int B, int D, int F, int T,
                         void* stream) {
  ALVQ_REQUIRE(X && Phi && status, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_TRY(check_mics(who, D));
  ALVQ_TRY(check_frames(who, T));
  const long nbins = (long)B * F;
  const BfCovArgs args{X, mask, (double2*)Phi, status, nbins, F, T};
  hipStream_t s = (hipStream_t)stream;
  if (T <= BF_WAVE_T) {
    const dim3 grid = capped_grid((nbins + BF_WAVES - 1) / BF_WAVES);
#define BF_CALL(N) hipLaunchKernelGGL((bf_cov_kernel<R, N, 1>), grid, dim3(BF_THREADS), 0, s, args)
    ALVQ_FOR_1_TO_8(D, BF_CALL)
#undef BF_CALL
  } else {
    const dim3 grid = capped_grid(nbins);
#define BF_CALL(N) hipLaunchKernelGGL((bf_cov_kernel<R, N, BF_WAVES>), grid, dim3(BF_THREADS), 0, s, args)
    ALVQ_FOR_1_TO_8(D, BF_CALL)
#undef BF_CALL
  }
  return check_launch(who);
}

extern "C" int alvq_spatial_covariance_f32(const float* X, const double* mask, double* Phi, int* status, int B, int D, int F, int T,
                                           void* stream) {
  return bf_cov_launch("alvq_spatial_covariance_f32", X, mask, Phi, status, B, D, F, T, stream);
}

extern "C" int alvq_spatial_covariance_f64(const double* X, const double* mask, double* Phi, int* status, int B, int D, int F, int T,
                                           void* stream) {
  return bf_cov_launch("alvq_spatial_covariance_f64", X, mask, Phi, status, B, D, F, T, stream);
}

extern "C" int alvq_steering_vectors_f64(const double* mics, const double* src, double* A, int* status, int B, int D, int F, double fs,
                                         int n_fft, double c, int ref, int mics_batched, void* stream) {
  const char* who = "alvq_steering_vectors_f64";
  ALVQ_REQUIRE(mics && src && A && status, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_TRY(check_mics(who, D));
  ALVQ_TRY(check_nfft(who, n_fft, F));
  ALVQ_TRY(check_rates(who, fs, c));
  ALVQ_REQUIRE(ref >= 0 && ref < D, ALVQ_EINVAL, "%s: ref=%d (need 0 <= ref < D = %d)", who, ref, D);
  hipLaunchKernelGGL(bf_steer_kernel, dim3(B), dim3(BF_THREADS), 0, (hipStream_t)stream, mics, src, (double2*)A, status, D, F,
                     mics_batched ? 3L * D : 0L, fs / (double)n_fft, c, ref);
  return check_launch(who);
}

extern "C" int alvq_beamform_weights_f64(const double* Phi_n, const double* Phi_s, const double* A, double* W, int* status, int B,
                                         int D, int F, int mode, int ref, double loading, void* stream) {
  const char* who = "alvq_beamform_weights_f64";
  ALVQ_REQUIRE(W && status, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_TRY(check_mics(who, D));
  ALVQ_REQUIRE(mode >= BF_DAS && mode <= BF_SOUDEN, ALVQ_EINVAL, "%s: mode=%d (need 0, 1 or 2)", who, mode);
  ALVQ_REQUIRE(ref >= 0 && ref < D, ALVQ_EINVAL, "%s: ref=%d (need 0 <= ref < D = %d)", who, ref, D);
  ALVQ_REQUIRE(std::isfinite(loading) && loading >= 0.0, ALVQ_EINVAL, "%s: loading=%g must be finite and >= 0", who, loading);
  ALVQ_REQUIRE((mode == BF_SOUDEN || A) && (mode == BF_DAS || Phi_n) && (mode != BF_SOUDEN || Phi_s), ALVQ_EINVAL,
               "%s: null pointer (mode 0 needs A, mode 1 Phi_n and A, mode 2 Phi_n and Phi_s)", who);
  const long nbins = (long)B * F;
  const BfWeightArgs args{(const double2*)Phi_n, (const double2*)Phi_s, (const double2*)A, (double2*)W, status, nbins, D, F, mode, ref,
                          loading};
  if (mode == BF_DAS)
    hipLaunchKernelGGL(bf_das_kernel, capped_grid((nbins * D + BF_THREADS - 1) / BF_THREADS), dim3(BF_THREADS), 0,
                       (hipStream_t)stream, args);
  else
    hipLaunchKernelGGL(bf_mvdr_kernel, capped_grid((nbins + BF_WAVES - 1) / BF_WAVES), dim3(BF_THREADS), 0, (hipStream_t)stream,
                       args);
  return check_launch(who);
}

extern "C" int alvq_beamform_gev_f64(const double* Phi_n, const double* Phi_s, double* W, double* RTF, double* gain, int* status,
                                     int B, int D, int F, int ref, double loading, void* stream) {
  const char* who = "alvq_beamform_gev_f64";
  ALVQ_REQUIRE(Phi_n && Phi_s && W && RTF && gain && status, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_TRY(check_mics(who, D));
  ALVQ_REQUIRE(ref >= 0 && ref < D, ALVQ_EINVAL, "%s: ref=%d (need 0 <= ref < D = %d)", who, ref, D);
  ALVQ_REQUIRE(std::isfinite(loading) && loading >= 0.0, ALVQ_EINVAL, "%s: loading=%g must be finite and >= 0", who, loading);
  const long nbins = (long)B * F;
  const BfGevArgs args{(const double2*)Phi_n, (const double2*)Phi_s, (double2*)W, (double2*)RTF, gain, status, nbins, D, ref, loading};
  hipLaunchKernelGGL(bf_gev_kernel, capped_grid((nbins + BF_WAVES - 1) / BF_WAVES), dim3(BF_THREADS), 0, (hipStream_t)stream, args);
  return check_launch(who);
}

template <typename R>
static int bf_apply_launch(const char* who, const R* X, const double* W, R* Y, int B, int D, int F, int T, void* stream) {
  ALVQ_REQUIRE(X && W && Y, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_TRY(check_mics(who, D));
  ALVQ_TRY(check_frames(who, T));
  const long nbins = (long)B * F, blocks = (nbins * T + BF_THREADS - 1) / BF_THREADS;
  const dim3 grid = capped_grid(blocks);
  hipStream_t s = (hipStream_t)stream;
#define BF_CALL(N) \
  hipLaunchKernelGGL((bf_apply_kernel<R, N>), grid, dim3(BF_THREADS), 0, s, (const void*)X, (const double2*)W, (void*)Y, nbins, F, T)
  ALVQ_FOR_1_TO_8(D, BF_CALL)
#undef BF_CALL
  return check_launch(who);
}

extern "C" int alvq_beamform_apply_f32(const float* X, const double* W, float* Y, int B, int D, int F, int T, void* stream) {
  return bf_apply_launch("alvq_beamform_apply_f32", X, W, Y, B, D, F, T, stream);
}

extern "C" int alvq_beamform_apply_f64(const double* X, const double* W, double* Y, int B, int D, int F, int T, void* stream) {
  return bf_apply_launch("alvq_beamform_apply_f64", X, W, Y, B, D, F, T, stream);
}
