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
// kMaxBlocks workgroups and strides over the bins (pairs, outputs) beyond, whole waves or whole workgroups at a time.
// No atomics anywhere, no host-side decision between the launches: the status is read on the device.
// What the launches cost: DESIGN.md.
// iva_check_kernel, iva_cov_kernel, iva_solve (and iva_solve_kernel) and iva_project_kernel live in csrc/iva_kernels.h, which
// csrc/ilrma.hip includes too; here the covariance's weights are the same in every bin (bin_stride = 0).
#include "iva_kernels.h"

namespace alvq {

// ----------------------------------------------------------------------------------------------------------------- activity
template <typename R, int D>
__global__ __launch_bounds__(kWave * D) void iva_activity_kernel(const void* X, const double2* W, const int* status, double* P, int F,
                                                                int T) {
  typedef typename Cplx<R>::type C;
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
    double2 y = cmul(w[0], x[0]);
#pragma unroll
    for (int d = 1; d < D; ++d) {
      const double2 q = cmul(w[d], x[d]);
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

// -------------------------------------------------------------------------------------------------------------------- masks
template <typename R, int K>
__global__ __launch_bounds__(IVA_THREADS) void iva_masks_kernel(const void* Y, double* M, long nbins, int F, int T) {
  typedef typename Cplx<R>::type C;
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
      else if (is_finite(s)) m = q[k] / s;
      M[at + k * chan_stride] = m;
    }
  }
}

}  // namespace alvq

using namespace alvq;

static int64_t iva_phi_bytes(int B, int D, int T) { return ((int64_t)8 * B * D * T + 15) / 16 * 16; }

extern "C" int64_t alvq_auxiva_workspace_bytes(int B, int D, int F, int T) {
  if (B < 1 || B > 65535 || F < 1 || (long)B * F > INT_MAX || D < 1 || D > kMaxMics || T < 1 || T > kMaxFrames) return -1;
  // p, then phi over it: (B, D, T) float64; the D weighted covariances of every bin: (B, F, D, D, D) complex128
  return iva_phi_bytes(B, D, T) + (int64_t)16 * B * F * D * D * D;
}

template <typename R>
static int iva_launch(const char* who, const R* X, const double* W0, double* W, R* Y, int* status, void* workspace, int B, int D, int F,
                      int T, int model, int iterations, int ref, double eps, void* stream) {
  ALVQ_REQUIRE(X && W && Y && status && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_TRY(check_mics(who, D));
  ALVQ_TRY(check_frames(who, T));
  ALVQ_REQUIRE(model == IVA_LAPLACE || model == IVA_GAUSS, ALVQ_EINVAL, "%s: model=%d (need 0 = laplace or 1 = gauss)", who, model);
  ALVQ_REQUIRE(iterations >= 0 && iterations <= IVA_MAX_ITERATIONS, ALVQ_EINVAL, "%s: iterations=%d (need 0 <= iterations <= 256)", who,
               iterations);
  ALVQ_REQUIRE(ref >= 0 && ref < D, ALVQ_EINVAL, "%s: ref=%d (need 0 <= ref < D = %d)", who, ref, D);
  ALVQ_REQUIRE(std::isfinite(eps) && eps >= 0.0, ALVQ_EINVAL, "%s: eps=%g must be finite and >= 0", who, eps);
  const long nbins = (long)B * F;
  hipStream_t s = (hipStream_t)stream;
  double* P = (double*)workspace;
  double2* Wd = (double2*)W;
  hipLaunchKernelGGL((iva_check_kernel<R>), capped_grid((nbins + IVA_WAVES - 1) / IVA_WAVES), dim3(IVA_THREADS), 0, s, (const void*)X,
                     (const double2*)W0, Wd, status, nbins, D, F, T);
  double2* V = (double2*)((char*)workspace + iva_phi_bytes(B, D, T));
  const dim3 tiles((unsigned)((T + IVA_TILE - 1) / IVA_TILE), (unsigned)B);
  const dim3 cov_grid = capped_grid((nbins * D + IVA_WAVES - 1) / IVA_WAVES), solve_grid = capped_grid((nbins + IVA_WAVES - 1) / IVA_WAVES);
  for (int it = 0; it < iterations; ++it) {
#define IVA_CALL(N) \
  hipLaunchKernelGGL((iva_activity_kernel<R, N>), tiles, dim3(kWave * N), 0, s, (const void*)X, (const double2*)Wd, (const int*)status, P, F, T)
    ALVQ_FOR_1_TO_8(D, IVA_CALL)
#undef IVA_CALL
    hipLaunchKernelGGL(iva_weights_kernel, dim3((unsigned)(B * D)), dim3(IVA_THREADS), 0, s, P, F, T, model, eps);
#define IVA_CALL(N) \
  hipLaunchKernelGGL((iva_cov_kernel<R, N>), cov_grid, dim3(IVA_THREADS), 0, s, (const void*)X, (const double*)P, (const int*)status, V, nbins, F, T, (long)T, 0L)
    ALVQ_FOR_1_TO_8(D, IVA_CALL)
#undef IVA_CALL
#define IVA_CALL(N) \
  hipLaunchKernelGGL((iva_solve_kernel<N, false>), solve_grid, dim3(IVA_THREADS), 0, s, (const double2*)V, Wd, status, nbins, (const double*)nullptr, F)
    ALVQ_FOR_1_TO_8(D, IVA_CALL)
#undef IVA_CALL
  }
#define IVA_CALL(N) \
  hipLaunchKernelGGL((iva_project_kernel<R, N>), capped_grid(nbins), dim3(IVA_THREADS), 0, s, (const void*)X, Wd, (void*)Y, status, nbins, F, T, ref)
  ALVQ_FOR_1_TO_8(D, IVA_CALL)
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
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_TRY(check_mics(who, K));
  ALVQ_TRY(check_frames(who, T));
  const long nbins = (long)B * F;
  const dim3 grid = capped_grid((nbins * T + IVA_THREADS - 1) / IVA_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define IVA_CALL(N) hipLaunchKernelGGL((iva_masks_kernel<R, N>), grid, dim3(IVA_THREADS), 0, s, (const void*)Y, M, nbins, F, T)
  ALVQ_FOR_1_TO_8(K, IVA_CALL)
#undef IVA_CALL
  return check_launch(who);
}

extern "C" int alvq_separation_masks_f32(const float* Y, double* M, int B, int K, int F, int T, void* stream) {
  return iva_masks_launch("alvq_separation_masks_f32", Y, M, B, K, F, T, stream);
}

extern "C" int alvq_separation_masks_f64(const double* Y, double* M, int B, int K, int F, int T, void* stream) {
  return iva_masks_launch("alvq_separation_masks_f64", Y, M, B, K, F, T, stream);
}
