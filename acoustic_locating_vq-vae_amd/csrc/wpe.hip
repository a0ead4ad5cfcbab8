// Weighted prediction error (WPE) dereverberation of complex spectrograms (Nakatani, Yoshioka, Kinoshita, Miyoshi, Juang
// 2010): per (item, frequency bin) a delayed linear prediction filter over the past frames of every microphone, estimated by
// iterated weighted least squares, is taken off the observed frames.  The definition is the comment on alvq_wpe_* in
// include/alvq.h; tests/helpers/wpe_ref.py restates it in numpy.  All arithmetic is float64; only Y is rounded.
//
// One workgroup of 256 threads owns one (b, f) bin through every iteration, in one launch; bins share nothing.  Its LDS holds
//   A   (M + D) x M complex: rows r < M the lower triangle of R, rows M + d the conjugated column d of P.  With
//       a_r = the stacked past x~_r (r < M) or the current frame x_d (r = M + d), A[r][c] = sum_t a_r[t] conj(a_c[t]) / lambda_t
//       for both.  The Cholesky factorisation runs on the M columns over all M + D rows, which leaves H = P^H L^-H in the
//       last D rows (the forward solve costs nothing extra); a column-wise back substitution turns them into W = H L^-1 = G^H
//       in place, and the filter is y_d[t] = x_d[t] - sum_i W[d][i] x~_i[t].
//   x   the bin's D rows of X widened to float64, q[t] = sum_d |y_d[t]|^2 and w[t] = 1 / lambda_t -- when 16 (D + 1) T bytes
//       fit next to A in the 160 KiB (ROW_LDS).  Otherwise x is re-read from X (only this workgroup reads those rows; they
//       stay in the L2) and q, w live in the caller's workspace.  y itself is never kept: the next iteration needs q alone,
//       and Y is written once, by the last filter pass, so a bin that fails in any iteration leaves with Y = X.
// Sums and their orders (they depend on the bin's sizes alone: a bin has the same bits in any batch and on any run):
//   A[r][c]  a wave per entry; lane l adds t = t0 + l, t0 + l + 64, ... rising, then the 64 lane sums meet in a butterfly
//   p_t      the frames of the window rising; the largest p_t is a maximum, which has no order
//   tr R     the diagonal rising;  Cholesky and the solves: column k = 0 .. M - 1 (back substitution M - 1 .. 0), one
//            subtraction per column on every entry;  the filter: i = 0 .. M - 1 rising
// The correlation build is the M^2 T hot loop and runs on plain float64 vector arithmetic, not on v_mfma_f64_16x16x4_f64: on
// gfx950 the float64 matrix rate equals the float64 vector rate, so the matrix instruction buys no arithmetic, while its
// 16 x 16 tiles would waste most of an M = 10 problem (55 wanted entries of 256) and bring a sum order of their own.  What the
// launch costs and where the time goes: DESIGN.md.
#include <cfloat>
#include <climits>
#include <cmath>

#include "array_wave.h"

namespace alvq {

constexpr int WPE_THREADS = 256;
constexpr int WPE_WAVES = WPE_THREADS / kWave;
constexpr int WPE_MAX_M = 64;
constexpr int WPE_LDS_LIMIT = 160 * 1024 - 256;      // dynamic LDS: the 160 KiB less the static reduction scratch

// status values of alvq_wpe_*
constexpr int WPE_BAD_POWER = 1;       // a non-finite value in the bin, or every frame's power 0
constexpr int WPE_BAD_PIVOT = 2;       // a Cholesky pivot <= 0 or not finite

struct WpeArgs {
  const void* X;
  void* Y;
  int* status;
  double* workspace;
  int B, D, F, T, taps, delay, iterations, psd_context;
  double eps, loading;
};

__host__ __device__ inline long wpe_matrix_doubles(int D, int taps) {
  const long M = (long)D * taps;
  return 2 * (M + D) * M;
}
// whether a bin's x, q and w fit in LDS next to A
inline bool wpe_row_in_lds(int D, int T, int taps) {
  return wpe_matrix_doubles(D, taps) * 8 + 16L * (D + 1) * T <= WPE_LDS_LIMIT;
}

template <typename R, bool ROW_LDS>
__global__ __launch_bounds__(WPE_THREADS) void wpe_kernel(WpeArgs a) {
  typedef typename Cplx<R>::type C;
  extern __shared__ __attribute__((aligned(16))) unsigned char wpe_smem[];
  __shared__ double s_max[WPE_WAVES];
  __shared__ int s_flag[WPE_WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int D = a.D, T = a.T, M = a.D * a.taps, rows = M + D;
  const long bin = blockIdx.x;
  const int b = (int)(bin / a.F), f = (int)(bin % a.F);
  // channel d of the bin: T consecutive complex values
  const long chan_stride = (long)a.F * T;
  const long row0 = ((long)b * D * a.F + f) * T;
  const C* Xg = (const C*)a.X + row0;
  C* Yg = (C*)a.Y + row0;

  double2* A = (double2*)wpe_smem;                                       // [rows][M]
  double2* xs = A + (long)rows * M;                                      // ROW_LDS: [D][T]
  double* q = ROW_LDS ? (double*)(xs + (long)D * T) : a.workspace + bin * 2L * T;
  double* w = q + T;

  auto ldx = [&](int d, int t) -> double2 {
    if (ROW_LDS) return xs[d * T + t];
    const C v = Xg[d * chan_stride + t];
    return make_double2((double)v.x, (double)v.y);
  };

  // ---- x into LDS, q_t = sum_d |x_d[t]|^2
  for (int t = tid; t < T; t += WPE_THREADS) {
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
      const C v = Xg[d * chan_stride + t];
      const double2 z = make_double2((double)v.x, (double)v.y);
      if (ROW_LDS) xs[d * T + t] = z;
      s += z.x * z.x + z.y * z.y;
    }
    q[t] = s;
  }
  __syncthreads();

  int fail = 0;
  for (int it = 0; it < a.iterations && !fail; ++it) {
    // ---- power over the clipped window, its maximum, the weights
    double pmax = 0.0;
    int bad = 0;
    for (int t = tid; t < T; t += WPE_THREADS) {
      const int lo = t - a.psd_context < 0 ? 0 : t - a.psd_context;
      const int hi = t + a.psd_context > T - 1 ? T - 1 : t + a.psd_context;
      double s = 0.0;
      for (int u = lo; u <= hi; ++u) s += q[u];
      const double p = s / (double)((long)D * (hi - lo + 1));
      if (!(p <= DBL_MAX)) bad = 1;                 // infinite or NaN
      else pmax = fmax(pmax, p);
      w[t] = p;
    }
    block_max_or<true>(pmax, bad, s_max, s_flag);
    if (bad || pmax == 0.0) {
      fail = WPE_BAD_POWER;
      break;
    }
    const double floor_p = a.eps * pmax;
    for (int t = tid; t < T; t += WPE_THREADS) w[t] = 1.0 / fmax(w[t], floor_p);      // a thread's own frames
    __syncthreads();

    // ---- A[r][c] = sum_t a_r[t] conj(a_c[t]) w_t: a wave per entry, c <= r where r < M
    for (int e = wv; e < rows * M; e += WPE_WAVES) {
      const int r = e / M, c = e - r * M;
      if (r < M && c > r) continue;
      const int dr = r < M ? r % D : r - M, sr = r < M ? a.delay + r / D : 0;
      const int dc = c % D, sc = a.delay + c / D;
      double2 acc = make_double2(0.0, 0.0);
      for (int t = (sr > sc ? sr : sc) + lane; t < T; t += kWave) {
        const double2 p = cmul_conj(ldx(dr, t - sr), ldx(dc, t - sc));
        const double wt = w[t];
        acc.x += p.x * wt;
        acc.y += p.y * wt;
      }
      acc.x = wave_sum(acc.x);
      acc.y = wave_sum(acc.y);
      if (lane == 0) A[r * M + c] = acc;
    }
    __syncthreads();

    // ---- diagonal loading by the mean of the diagonal
    double tr = 0.0;
    for (int i = 0; i < M; ++i) tr += A[i * M + i].x;
    __syncthreads();                                // every thread has the trace before the diagonal changes
    const double load = a.loading * (tr / (double)M);
    if (tid < M) A[tid * M + tid].x += load;
    __syncthreads();

    // ---- Cholesky over the M columns of all rows: column k of L (and of H) replaces column k of A, the pivot stays on the
    //      diagonal (l_kk is its square root wherever it is needed)
    for (int k = 0; k < M; ++k) {
      const double piv = A[k * M + k].x;
      if (!(piv > 0.0 && piv <= DBL_MAX)) {         // the same value in every thread
        fail = WPE_BAD_PIVOT;
        break;
      }
      const double l = sqrt(piv);
      for (int r = k + 1 + tid; r < rows; r += WPE_THREADS) {
        double2 v = A[r * M + k];
        v.x /= l;
        v.y /= l;
        A[r * M + k] = v;
      }
      __syncthreads();
      const int wd = M - k - 1, n = (rows - k - 1) * wd;
      for (int e = tid; e < n; e += WPE_THREADS) {
        const int r = k + 1 + e / wd, c = k + 1 + e % wd;
        if (c > r) continue;
        const double2 p = cmul_conj(A[r * M + k], A[c * M + k]);
        double2 v = A[r * M + c];
        v.x -= p.x;
        v.y -= p.y;
        A[r * M + c] = v;
      }
      __syncthreads();
    }
    if (fail) break;

    // ---- W L = H from the last column back: W[d][k] = H[d][k] / l_kk, then H[d][j] -= W[d][k] L[k][j] for j < k
    for (int k = M - 1; k >= 0; --k) {
      const double l = sqrt(A[k * M + k].x);
      if (tid < D) {
        double2 v = A[(M + tid) * M + k];
        v.x /= l;
        v.y /= l;
        A[(M + tid) * M + k] = v;
      }
      __syncthreads();
      for (int e = tid; e < D * k; e += WPE_THREADS) {
        const int d = e / k, j = e - d * k;
        const double2 p = cmul(A[(M + d) * M + k], A[k * M + j]);
        double2 v = A[(M + d) * M + j];
        v.x -= p.x;
        v.y -= p.y;
        A[(M + d) * M + j] = v;
      }
      __syncthreads();
    }

    // ---- filter: y_d[t] = x_d[t] - sum_i W[d][i] x~_i[t]; the next iteration's q, or Y after the last
    const bool last = it == a.iterations - 1;
    for (int t = tid; t < T; t += WPE_THREADS) {
      double s = 0.0;
      for (int d = 0; d < D; ++d) {
        double2 y = ldx(d, t);
        const int kmax = t - a.delay + 1 < a.taps ? t - a.delay + 1 : a.taps;        // taps whose frame exists
        for (int k = 0; k < kmax; ++k)
          for (int d2 = 0; d2 < D; ++d2) {
            const double2 p = cmul(A[(M + d) * M + k * D + d2], ldx(d2, t - a.delay - k));
            y.x -= p.x;
            y.y -= p.y;
          }
        s += y.x * y.x + y.y * y.y;
        if (last) {
          C out;
          out.x = (R)y.x;
          out.y = (R)y.y;
          Yg[d * chan_stride + t] = out;
        }
      }
      if (!last) q[t] = s;
    }
    __syncthreads();
  }

  if (fail)                                         // Y = X for the whole bin, bit for bit
    for (int t = tid; t < T; t += WPE_THREADS)
      for (int d = 0; d < D; ++d) Yg[d * chan_stride + t] = Xg[d * chan_stride + t];
  if (tid == 0) a.status[bin] = fail;
}

}  // namespace alvq

using namespace alvq;

static int wpe_check_dims(const char* who, int B, int D, int F, int T, int taps) {
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_REQUIRE(D >= 1 && D <= kMaxMics && taps >= 1 && (long)D * taps <= WPE_MAX_M, ALVQ_EINVAL,
               "%s: D=%d taps=%d (need 1 <= D <= 8, taps >= 1, D taps <= 64)", who, D, taps);
  return check_frames(who, T);
}

// q and w of every bin (2 T doubles each) where a bin's rows do not fit in LDS; nothing otherwise
extern "C" int64_t alvq_wpe_workspace_bytes(int B, int D, int F, int T, int taps) {
  if (B < 1 || B > 65535 || F < 1 || (long)B * F > INT_MAX || D < 1 || D > kMaxMics || taps < 1 || (long)D * taps > WPE_MAX_M ||
      T < 1 || T > kMaxFrames)
    return -1;
  return wpe_row_in_lds(D, T, taps) ? 0 : (int64_t)B * F * 2 * T * 8;
}

template <typename R>
static int wpe_launch(const char* who, const R* X, R* Y, int* status, void* workspace, int B, int D, int F, int T, int taps, int delay,
                      int iterations, int psd_context, double eps, double loading, void* stream) {
  ALVQ_REQUIRE(X && Y && status, ALVQ_EINVAL, "%s: null pointer", who);
  const int rc = wpe_check_dims(who, B, D, F, T, taps);
  if (rc != ALVQ_OK) return rc;
  ALVQ_REQUIRE(delay >= 0 && delay <= 64 && iterations >= 1 && iterations <= 16 && psd_context >= 0 && psd_context <= 64, ALVQ_EINVAL,
               "%s: delay=%d iterations=%d psd_context=%d (need 0 <= delay <= 64, 1 <= iterations <= 16, 0 <= psd_context <= 64)",
               who, delay, iterations, psd_context);
  ALVQ_REQUIRE(std::isfinite(eps) && eps >= 0.0 && std::isfinite(loading) && loading >= 0.0, ALVQ_EINVAL,
               "%s: eps=%g loading=%g must be finite and >= 0", who, eps, loading);
  const bool row_lds = wpe_row_in_lds(D, T, taps);
  ALVQ_REQUIRE(row_lds || workspace, ALVQ_EINVAL, "%s: null workspace (alvq_wpe_workspace_bytes is not 0 for these sizes)", who);
  const WpeArgs args{X, Y, status, (double*)workspace, B, D, F, T, taps, delay, iterations, psd_context, eps, loading};
  const size_t lds = (size_t)wpe_matrix_doubles(D, taps) * 8 + (row_lds ? 16 * (size_t)(D + 1) * T : 0);
  static DeviceOnce attr;  // once per device (not inside a graph capture on every call)
  if (attr.need()) {
    (void)hipFuncSetAttribute((const void*)wpe_kernel<R, true>, hipFuncAttributeMaxDynamicSharedMemorySize, WPE_LDS_LIMIT);
    (void)hipFuncSetAttribute((const void*)wpe_kernel<R, false>, hipFuncAttributeMaxDynamicSharedMemorySize, WPE_LDS_LIMIT);
  }
  const dim3 grid((unsigned)((long)B * F));
  if (row_lds)
    hipLaunchKernelGGL((wpe_kernel<R, true>), grid, dim3(WPE_THREADS), lds, (hipStream_t)stream, args);
  else
    hipLaunchKernelGGL((wpe_kernel<R, false>), grid, dim3(WPE_THREADS), lds, (hipStream_t)stream, args);
  return check_launch(who);
}

extern "C" int alvq_wpe_f32(const float* X, float* Y, int* status, void* workspace, int B, int D, int F, int T, int taps, int delay,
                            int iterations, int psd_context, double eps, double loading, void* stream) {
  return wpe_launch("alvq_wpe_f32", X, Y, status, workspace, B, D, F, T, taps, delay, iterations, psd_context, eps, loading, stream);
}

extern "C" int alvq_wpe_f64(const double* X, double* Y, int* status, void* workspace, int B, int D, int F, int T, int taps, int delay,
                            int iterations, int psd_context, double eps, double loading, void* stream) {
  return wpe_launch("alvq_wpe_f64", X, Y, status, workspace, B, D, F, T, taps, delay, iterations, psd_context, eps, loading, stream);
}
