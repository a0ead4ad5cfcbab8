// cACGMM spatial clustering of a microphone array's complex spectrograms (the complex angular central Gaussian mixture model;
// Ito, Araki, Nakatani, EUSIPCO 2016): time-frequency masks for K classes from D microphones, K and D independent.  The
// definitions are the comment on alvq_cacgmm_* in include/alvq.h; tests/helpers/cacgmm_ref.py restates them in numpy.  All
// arithmetic is float64.  The state between iterations is gamma and q, which live in the outputs masks and quadratic.
//
// cac_check_kernel<R>     one pass over X, init and quadratic0, a wave a (b, f) bin (four bins a workgroup), a lane a frame: the
//                     bin's status, and gamma = init, q = quadratic0 or 1 copied into the outputs.
// cac_prior_kernel        step 1, iva_activity_kernel's structure: the grid runs over (frame tiles of CAC_TILE = 64, b); a
//                     workgroup has K waves, wave k owns class k and a lane a frame t; it walks f rising, adds gamma where the
//                     bin's status is 0 (a select, no branch: four loads in flight) and counts F0.  The order over f is fixed, so
//                     an item has the same bits alone or in a batch.  It stores the prior and, into the workspace, its
//                     logarithm, which every one of the F bins of the E-step would otherwise take again.
// cac_cov_kernel<R, D>    step 2, the pass over X.  A wave owns a pair (bin, k), four pairs a workgroup, no LDS and no barrier.
//                     iva_cov_kernel's layout: lane l adds the frames t = l, l + 64, ... rising to D^2 float64 accumulators (the
//                     lower triangle, the diagonal real) with the weight gamma / (q |x|^2), and to sum_t gamma; wave_sum brings
//                     the lane sums together; lane r D + c stores entry (r, c) of B_k (above the diagonal the exact conjugate;
//                     I for a class without weight) into the pair's 16 D^2 bytes of workspace.
// cac_eig_kernel<D>       step 2, the decomposition.  A wave a pair in herm_eig's lane-per-entry layout, four a workgroup, no
//                     LDS, no barrier.  The floor, the normalisation and logdet are taken by every lane from shuffled copies of
//                     the eigenvalues in ascending order (the same bits in every lane).  It stores row `rank` of
//                     lambda^-1/2 V^H over B_k (every lane has read its entry before any lane writes) and logdet, and in the
//                     last iteration cov.  A failure sets the bin's status to 2: the K waves of a bin may all write it, and
//                     only ever this one value.
// cac_estep_kernel<R, D>  step 3.  A workgroup of 256 threads a bin; the K matrices lambda^-1/2 V^H and logdets of the bin go to
//                     LDS once (8 KB at K = D = 8; every lane reads the same address: a broadcast), then a thread a frame
//                     t = tid, tid + 256, ...: D loads of X coalesced along t, K D^2 complex multiply-adds, the softmax, and the
//                     stores of gamma and q.  K is a run-time size, so the K values l_k of a frame wait in a private LDS column
//                     (ls[k][tid], 16 KB) rather than in an array that would have to be indexed at run time: no scratch.  A bin
//                     whose status is not 0 gets masks = 1 / K and quadratic = 1, and cov = I in the last iteration.
// TWO DIVERGENCES from the suggested plan.
//   z = x / sqrt(|x|^2) is never formed.  z z^H = x x^H / |x|^2 enters the M-step through the frame's weight, and
//   |v^H z|^2 = |v^H x|^2 / |x|^2 the E-step through one division per class: one division where 2 D divisions and a square
//   root per frame and pass would stand, each of them a dozen float64 instructions.
//   The M-step is two launches, 1 + 4 iterations in all, with B_k passing through the workspace slot that lambda^-1/2 V^H
//   then takes.  Fused -- accumulate, wave_sum and herm_eig on the same wave, as suggested and as built first -- the kernel
//   keeps the D^2 accumulators' registers for the whole decomposition (134 VGPRs at D = 4, 256 + 50 AGPRs at D = 8: three waves
//   and one wave a SIMD), and the decomposition is a chain of dependent shuffles, divisions and square roots that only other
//   waves can hide: measured 0.407 ms of a 0.734 ms iteration at (B, D, K, F, T) = (64, 4, 3, 201, 500) and 0.320 ms of 0.417 ms
//   at (8, 8, 3, 201, 500), where 4824 matrices then ran five deep on 1024 SIMDs.  The bits are the same either way.
// Every grid but cac_prior_kernel's (at most 1024 x 65535) is capped at kMaxBlocks workgroups and strides over the bins
// (pairs) beyond, whole waves or whole workgroups at a time.  No atomics anywhere, no host-side decision between the launches: the
// status is read on the device.  v_mfma_f64 is not used, for the reason csrc/wpe.hip gives.
// What the launches cost: DESIGN.md.
#include <cfloat>
#include <climits>
#include <cmath>

#include "array_wave.h"
#include "herm_eig.h"

namespace alvq {

constexpr int CAC_THREADS = 256;
constexpr int CAC_WAVES = CAC_THREADS / kWave;
constexpr int CAC_TILE = 64;               // the frames of a workgroup of cac_prior_kernel: a lane each, in every wave
constexpr int CAC_MAX_K = 8;
constexpr int CAC_MAX_ITERATIONS = 256;

constexpr int CAC_BAD_INPUT = 1;           // a non-finite X or |x|^2, a negative or non-finite init, a quadratic0 not > 0 and finite
constexpr int CAC_BAD_EIG = 2;             // herm_eig's status, or a lambda_max that is not > 0 and finite

// -------------------------------------------------------------------------------------------------------------------- check
template <typename R>
__global__ __launch_bounds__(CAC_THREADS) void cac_check_kernel(const void* X, const double* init, const double* q0, double* gamma,
                                                                 double* quad, int* status, long nbins, int D, int K, int F, int T) {
  typedef typename Cplx<R>::type C;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long chan_stride = (long)F * T;
  for (long bin = (long)blockIdx.x * CAC_WAVES + wv; bin < nbins; bin += (long)gridDim.x * CAC_WAVES) {
    const int b = (int)(bin / F), f = (int)(bin % F);
    const C* xg = (const C*)X + ((long)b * D * F + f) * T;
    const long at = ((long)b * K * F + f) * T;
    int bad = 0;
    for (int t = lane; t < T; t += kWave) {
      double n = 0.0;
      for (int d = 0; d < D; ++d) {
        const C v = xg[d * chan_stride + t];
        const double re = (double)v.x, im = (double)v.y;
        if (!is_finite(re) || !is_finite(im)) bad = 1;
        n += re * re + im * im;
      }
      if (!is_finite(n)) bad = 1;
      for (int k = 0; k < K; ++k) {        // a thread rewrites what it read itself: init may be masks, quadratic0 quadratic
        const long i = at + k * chan_stride + t;
        const double g = init[i], q = q0 ? q0[i] : 1.0;
        if (!(g >= 0.0 && g <= DBL_MAX)) bad = 1;
        if (!(q > 0.0 && q <= DBL_MAX)) bad = 1;
        gamma[i] = g;
        quad[i] = q;
      }
    }
    bad = wave_or(bad);
    if (lane == 0) status[bin] = bad ? CAC_BAD_INPUT : 0;
  }
}

// ------------------------------------------------------------------------------------------------------------------- priors
__global__ __launch_bounds__(kWave * CAC_MAX_K) void cac_prior_kernel(const double* gamma, const int* status, double* prior,
                                                                       double* logprior, int K, int F, int T) {
  const int lane = threadIdx.x & 63;
  const int k = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));          // wave k of the workgroup owns class k
  const int b = blockIdx.y, t = blockIdx.x * CAC_TILE + lane;
  const bool live = t < T;
  const double* g = gamma + ((long)b * K + k) * F * T + (live ? t : T - 1);        // a lane past the row reads its last frame
  double p = 0.0;
  int f0 = 0;
#pragma unroll 4
  for (int f = 0; f < F; ++f) {
    const bool ok = status[(long)b * F + f] == 0;      // the same in every lane; what another bin holds is loaded and dropped
    const double s = p + g[(long)f * T];
    p = ok ? s : p;
    f0 += ok ? 1 : 0;
  }
  if (live) {
    const double pr = f0 ? p / (double)f0 : 1.0 / (double)K;
    prior[((long)b * K + k) * T + t] = pr;
    logprior[((long)b * K + k) * T + t] = log(pr);
  }
}

// ------------------------------------------------------------------------------------------------------------------- M-step: B_k
template <typename R, int D>
__global__ __launch_bounds__(CAC_THREADS) void cac_cov_kernel(const void* X, const double* gamma, const double* quad,
                                                               const int* status, double2* A, long nbins, int K, int F, int T) {
  typedef typename Cplx<R>::type C;
  constexpr int NA = D * D;                            // D real diagonal sums and D (D - 1) / 2 complex ones below it
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long chan_stride = (long)F * T;
  // the grid is capped: a wave strides over its (bin, k) pairs, whole, and meets no barrier anywhere
  for (long e = (long)blockIdx.x * CAC_WAVES + wv; e < nbins * K; e += (long)gridDim.x * CAC_WAVES) {
    const long bin = e / K;
    const int k = (int)(e - bin * K);
    if (status[bin] != 0) continue;
    const int b = (int)(bin / F), f = (int)(bin % F);
    const C* xg = (const C*)X + ((long)b * D * F + f) * T;
    const long at = (((long)b * K + k) * F + f) * T;

    double acc[NA];
#pragma unroll
    for (int n = 0; n < NA; ++n) acc[n] = 0.0;
    double sg = 0.0;
    for (int t = lane; t < T; t += kWave) {
      C v[D];
#pragma unroll
      for (int d = 0; d < D; ++d) v[d] = xg[d * chan_stride + t];
      const double g = gamma[at + t], q = quad[at + t];
      double2 x[D];
      double nrm = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        x[d] = make_double2((double)v[d].x, (double)v[d].y);
        nrm += x[d].x * x[d].x + x[d].y * x[d].y;
      }
      const bool live = nrm > 0.0;                     // a silent frame has weight 0 in both sums
      const double w = live ? g / (q * nrm) : 0.0;
      sg += live ? g : 0.0;
      // a frame's term c = x_i conj(x_j) and acc = fma(w, c, acc): iva_cov_kernel's rule
      int n = 0;
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          const double re = fma(x[i].y, x[j].y, x[i].x * x[j].x);
          acc[n] = fma(w, re, acc[n]);
          ++n;
          if (j < i) {
            const double im = x[i].y * x[j].x - x[i].x * x[j].y;
            acc[n] = fma(w, im, acc[n]);
            ++n;
          }
        }
    }
#pragma unroll
    for (int n = 0; n < NA; ++n) acc[n] = wave_sum(acc[n]);
    sg = wave_sum(sg);
    double re = 0.0, im = 0.0;                         // lane i D + j picks its entry
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
          im = -si;                                    // the exact conjugate: a product and a division keep the sign
        }
      }
    if (lane < D * D) {
      const bool diag = lane / D == lane % D;
      double2 a = make_double2(diag ? 1.0 : 0.0, 0.0);                     // a class without weight keeps B_k = I
      if (sg > 0.0) a = make_double2((double)D * re / sg, diag ? 0.0 : (double)D * im / sg);
      A[e * (D * D) + lane] = a;
    }
  }
}

// ------------------------------------------------------------------------------------------------- M-step: the decomposition
template <int D>
__global__ __launch_bounds__(CAC_THREADS) void cac_eig_kernel(int* status, double2* A, double* logdet, double2* cov, long nbins, int K,
                                                               double floor, int last) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane >> 3, c = lane & 7;
  const bool in = r < D && c < D;
  const int at = in ? r * D + c : 0;                   // a lane outside the block loads entry 0 and drops it
  // the grid is capped: a wave strides over its (bin, k) pairs, whole, and meets no barrier anywhere
  for (long e = (long)blockIdx.x * CAC_WAVES + wv; e < nbins * K; e += (long)gridDim.x * CAC_WAVES) {
    const long bin = e / K;
    if (status[bin] != 0) continue;                    // 2 from another wave of this launch: the E-step drops the bin anyway
    double2 a = A[e * (D * D) + at];
    if (!in) a = make_double2(0.0, 0.0);
    double2 v;
    const HermEig eg = herm_eig(a, v, D, lane);
    int fail = eg.status ? CAC_BAD_EIG : 0;            // the same in every lane, as everything below
    int col[D];                                        // the column of the j-th eigenvalue in ascending order
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const unsigned long long m = __ballot(r == 0 && c < D && eg.rank == j);
      col[j] = m ? __ffsll((long long)m) - 1 : 0;
    }
    const double lmax = __shfl(eg.lam, col[D - 1], 64);
    if (!(lmax > 0.0 && lmax <= DBL_MAX)) fail = CAC_BAD_EIG;
    if (fail) {
      if (lane == 0) status[bin] = CAC_BAD_EIG;
      continue;
    }
    const double low = floor * lmax;
    double lam[D];
    double total = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      lam[j] = fmax(__shfl(eg.lam, col[j], 64), low);
      total = j == 0 ? lam[0] : total + lam[j];
    }
    double ld = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      lam[j] = lam[j] * (double)D / total;
      const double lg = log(lam[j]);
      ld = j == 0 ? lg : ld + lg;
    }
    const double mine = fmax(eg.lam, low) * (double)D / total;             // the lane's column
    const double root = sqrt(mine);
    // row i = rank of lambda^-1/2 V^H: entry (i, d) = conj(V[d][i]) / sqrt(lambda_i)
    if (in) A[(e * D + eg.rank) * D + r] = make_double2(v.x / root, -(v.y / root));
    if (lane == 0) logdet[e] = ld;
    if (last) {
      // cov[r][c] = sum_i lambda_i V[r][i] conj(V[c][i]), i in ascending order from the first term; the product's parts as in
      // the frame terms, so that (c, r) is the exact conjugate of (r, c) and the diagonal's imaginary part is +0
      double2 s = make_double2(0.0, 0.0);
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 p = cshfl(v, 8 * r + col[j]), o = cshfl(v, 8 * c + col[j]);
        const double pr = lam[j] * (p.x * o.x + p.y * o.y), pi = lam[j] * (p.y * o.x - p.x * o.y);
        s = j == 0 ? make_double2(pr, pi) : make_double2(s.x + pr, s.y + pi);
      }
      if (in) cov[(e * D + r) * D + c] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- E-step
template <typename R, int D>
__global__ __launch_bounds__(CAC_THREADS) void cac_estep_kernel(const void* X, const double* prior, const double* logprior,
                                                                 const double2* A, const double* logdet, const int* status,
                                                                 double* gamma, double* quad, double2* cov, long nbins, int K, int F,
                                                                 int T, int last) {
  typedef typename Cplx<R>::type C;
  __shared__ double2 As[CAC_MAX_K * D * D];
  __shared__ double lds[CAC_MAX_K];
  __shared__ double ls[CAC_MAX_K][CAC_THREADS];        // a private column a thread: the frame's l_k, then exp(l_k - max)
  const int tid = threadIdx.x;
  const long chan_stride = (long)F * T;
  const int na = K * D * D;
  for (long bin = blockIdx.x; bin < nbins; bin += gridDim.x) {
    const int b = (int)(bin / F), f = (int)(bin % F);
    const long at = ((long)b * K * F + f) * T;
    if (status[bin] != 0) {                            // the same in the whole workgroup: nobody writes a status in this launch
      const double even = 1.0 / (double)K;
      for (int t = tid; t < T; t += CAC_THREADS)
        for (int k = 0; k < K; ++k) {
          gamma[at + k * chan_stride + t] = even;
          quad[at + k * chan_stride + t] = 1.0;
        }
      if (last)
        for (int i = tid; i < na; i += CAC_THREADS) {
          const int rc = i % (D * D);
          cov[bin * na + i] = make_double2(rc / D == rc % D ? 1.0 : 0.0, 0.0);
        }
      continue;
    }
    for (int i = tid; i < na; i += CAC_THREADS) As[i] = A[bin * na + i];
    if (tid < K) lds[tid] = logdet[bin * K + tid];
    __syncthreads();
    const C* xg = (const C*)X + ((long)b * D * F + f) * T;
    const double* pg = prior + (long)b * K * T;
    const double* lg = logprior + (long)b * K * T;
    for (int t = tid; t < T; t += CAC_THREADS) {
      double2 x[D];
      double nrm = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const C v = xg[d * chan_stride + t];
        x[d] = make_double2((double)v.x, (double)v.y);
      }
#pragma unroll
      for (int d = 0; d < D; ++d) nrm += x[d].x * x[d].x + x[d].y * x[d].y;
      const bool live = nrm > 0.0;
      double top = -INFINITY;
      for (int k = 0; k < K; ++k) {
        const double2* ak = As + k * (D * D);
        double qs = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
          double2 y = cmul(ak[i * D], x[0]);        // d rising from the first product
#pragma unroll
          for (int d = 1; d < D; ++d) {
            const double2 p = cmul(ak[i * D + d], x[d]);
            y.x += p.x;
            y.y += p.y;
          }
          qs += y.x * y.x + y.y * y.y;
        }
        const double qk = fmax(qs / nrm, DBL_MIN);
        const double l = lg[(long)k * T + t] - lds[k] - (double)D * log(qk);
        ls[k][tid] = l;
        top = fmax(top, l);
        quad[at + k * chan_stride + t] = live ? qk : 1.0;
      }
      double total = 0.0;
      for (int k = 0; k < K; ++k) {
        const double ex = exp(ls[k][tid] - top);
        ls[k][tid] = ex;
        total += ex;
      }
      const bool flat = !(top > -DBL_MAX);             // every l_k is -inf: no class has a prior here
      for (int k = 0; k < K; ++k) {
        double g = flat ? 1.0 / (double)K : ls[k][tid] / total;
        if (!live) g = pg[(long)k * T + t];            // a silent frame keeps its prior
        gamma[at + k * chan_stride + t] = g;
      }
    }
    __syncthreads();                                   // As and lds are free for the next bin
  }
}

}  // namespace alvq

using namespace alvq;

static bool cac_dims_ok(int B, int D, int K, int F, int T) {
  return B >= 1 && B <= 65535 && F >= 1 && (long)B * F <= INT_MAX && D >= 2 && D <= kMaxMics && K >= 1 && K <= CAC_MAX_K && T >= 1 &&
         T <= kMaxFrames;
}

extern "C" int64_t alvq_cacgmm_workspace_bytes(int B, int D, int K, int F, int T) {
  if (!cac_dims_ok(B, D, K, F, T)) return -1;
  // B_k, then lambda^-1/2 V^H over it, of every class of every bin: (B, F, K, D, D) complex128; their logdets: (B, F, K)
  // float64; the logarithms of the priors: (B, K, T) float64
  return (int64_t)16 * B * F * K * D * D + (int64_t)8 * B * F * K + (int64_t)8 * B * K * T;
}

template <typename R>
static int cac_launch(const char* who, const R* X, const double* init, const double* quadratic0, double* masks, double* prior,
                      double* cov, double* quadratic, int* status, void* workspace, int B, int D, int K, int F, int T, int iterations,
                      double floor, void* stream) {
  ALVQ_REQUIRE(X && init && masks && prior && cov && quadratic && status && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_TRY(check_bins(who, B, F));
  ALVQ_TRY(check_mics(who, D, 2));
  ALVQ_REQUIRE(K >= 1 && K <= CAC_MAX_K, ALVQ_EINVAL, "%s: K=%d (need 1 <= K <= 8)", who, K);
  ALVQ_TRY(check_frames(who, T));
  ALVQ_REQUIRE(iterations >= 1 && iterations <= CAC_MAX_ITERATIONS, ALVQ_EINVAL, "%s: iterations=%d (need 1 <= iterations <= 256)",
               who, iterations);
  ALVQ_REQUIRE(floor >= 0.0 && floor <= 1.0, ALVQ_EINVAL, "%s: floor=%g must be in [0, 1]", who, floor);
  const long nbins = (long)B * F;
  hipStream_t s = (hipStream_t)stream;
  double2* A = (double2*)workspace;
  double* logdet = (double*)((char*)workspace + (int64_t)16 * nbins * K * D * D);
  double* logprior = logdet + nbins * K;
  hipLaunchKernelGGL((cac_check_kernel<R>), capped_grid((nbins + CAC_WAVES - 1) / CAC_WAVES), dim3(CAC_THREADS), 0, s, (const void*)X, init,
                     quadratic0, masks, quadratic, status, nbins, D, K, F, T);
  const dim3 tiles((unsigned)((T + CAC_TILE - 1) / CAC_TILE), (unsigned)B);
  const dim3 m_grid = capped_grid((nbins * K + CAC_WAVES - 1) / CAC_WAVES), e_grid = capped_grid(nbins);
  for (int it = 0; it < iterations; ++it) {
    const int last = it == iterations - 1;
    hipLaunchKernelGGL(cac_prior_kernel, tiles, dim3(kWave * K), 0, s, (const double*)masks, (const int*)status, prior, logprior, K, F,
                       T);
#define CAC_CALL(N)                                                                                                      \
  hipLaunchKernelGGL((cac_cov_kernel<R, N>), m_grid, dim3(CAC_THREADS), 0, s, (const void*)X, (const double*)masks,     \
                     (const double*)quadratic, (const int*)status, A, nbins, K, F, T)
    ALVQ_FOR_2_TO_8(D, CAC_CALL)
#undef CAC_CALL
#define CAC_CALL(N) \
  hipLaunchKernelGGL((cac_eig_kernel<N>), m_grid, dim3(CAC_THREADS), 0, s, status, A, logdet, (double2*)cov, nbins, K, floor, last)
    ALVQ_FOR_2_TO_8(D, CAC_CALL)
#undef CAC_CALL
#define CAC_CALL(N)                                                                                                                   \
  hipLaunchKernelGGL((cac_estep_kernel<R, N>), e_grid, dim3(CAC_THREADS), 0, s, (const void*)X, (const double*)prior,               \
                     (const double*)logprior, (const double2*)A, \
                     (const double*)logdet, (const int*)status, masks, quadratic, (double2*)cov, nbins, K, F, T, last)
    ALVQ_FOR_2_TO_8(D, CAC_CALL)
#undef CAC_CALL
  }
  return check_launch(who);
}

extern "C" int alvq_cacgmm_f32(const float* X, const double* init, const double* quadratic0, double* masks, double* prior, double* cov,
                               double* quadratic, int* status, void* workspace, int B, int D, int K, int F, int T, int iterations,
                               double floor, void* stream) {
  return cac_launch("alvq_cacgmm_f32", X, init, quadratic0, masks, prior, cov, quadratic, status, workspace, B, D, K, F, T, iterations,
                    floor, stream);
}

extern "C" int alvq_cacgmm_f64(const double* X, const double* init, const double* quadratic0, double* masks, double* prior, double* cov,
                               double* quadratic, int* status, void* workspace, int B, int D, int K, int F, int T, int iterations,
                               double floor, void* stream) {
  return cac_launch("alvq_cacgmm_f64", X, init, quadratic0, masks, prior, cov, quadratic, status, workspace, B, D, K, F, T, iterations,
                    floor, stream);
}
