// Exact t-SNE (sklearn.manifold.TSNE(method="exact", n_components=2) semantics) of code-index sequences: the analysis that asks
// whether the RIR codes of an echoed utterance encode where the source was.
//
// Kernels, every sum in one fixed order (no atomics), so results are bitwise reproducible:
//   sqdist_kernel      64 x 64 output tile per workgroup, int32 code rows staged in LDS in chunks of 32 positions; a thread
//                      counts matches for 4 x 4 pairs: d2 = 2 (L - matches), the squared distance of the one-hot expansions.
//   search_kernel      one 1024-thread workgroup per row: the perplexity binary search for beta in fp64 over the row's fp32
//                      distances, held in registers (25 per thread) and LDS past j = 25600, so the up to 100 steps read it once;
//                      the workgroup then overwrites its own row with the conditional P.
//   symmetrize_kernel  tile pair (I, J), I <= J: both 64 x 64 tiles staged in LDS, then P[i][j] = P[j][i] = Pc[i][j] + Pc[j][i]
//                      (one fp32 add, commutative: exactly symmetric).
//   rowsum_kernel      one wave per row: sum of the off-diagonal P in fp64; reduce_kernel (one workgroup) sums the rows.
//   normalize_kernel   one workgroup per row: P = max(P / max(total, eps), eps) off the diagonal.
//   numsum_kernel      descent pass (a): one wave per row, sum_j != i 1 / (1 + |y_i - y_j|^2) in fp64; reduce_kernel -> Z.
//   grad_kernel        descent pass (b)+(c): one wave per row reads its row of P (coalesced), forms grad_i (and the KL terms on
//                      the call's last iteration), and lane 0 applies gains / momentum / step, writing the new y_i into the
//                      OTHER ping-pong buffer, so no row's new y is seen by another row's gradient in the same iteration.
// One descent call enqueues 3 launches per iteration (+ 2 for its statistics) on one stream: a linear chain, capturable.
#include <cmath>

#include "alvq_common.h"

namespace alvq {

constexpr int TS_TILE = 64;   // sqdist / symmetrize tile edge
constexpr int TS_LC = 32;     // code positions per LDS chunk
constexpr int TS_MAX_N = 65536;
constexpr int TS_MAX_L = 4096;
constexpr double TS_EPS = 2.220446049250313e-16;  // float64 machine epsilon (sklearn's MACHINE_EPSILON)

__global__ __launch_bounds__(256) void sqdist_kernel(const int* __restrict__ codes, float* __restrict__ d2, int N, int L) {
  __shared__ int ci[TS_TILE][TS_LC + 1];
  __shared__ int cj[TS_TILE][TS_LC + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int I0 = blockIdx.y * TS_TILE, J0 = blockIdx.x * TS_TILE;
  int m[4][4] = {};
  for (int l0 = 0; l0 < L; l0 += TS_LC) {
    for (int e = tid; e < TS_TILE * TS_LC; e += 256) {
      const int r = e / TS_LC, l = e % TS_LC;
      const bool in_l = l0 + l < L;
      ci[r][l] = (I0 + r < N && in_l) ? codes[(int64_t)(I0 + r) * L + l0 + l] : 0;
      cj[r][l] = (J0 + r < N && in_l) ? codes[(int64_t)(J0 + r) * L + l0 + l] : 0;
    }
    __syncthreads();
    const int lim = min(TS_LC, L - l0);
    for (int l = 0; l < lim; ++l) {
      int a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = ci[ty * 4 + r][l];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = cj[tx + 16 * c][l];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) m[r][c] += (a[r] == b[c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = I0 + ty * 4 + r;
    if (i >= N) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = J0 + tx + 16 * c;
      if (j < N) d2[(int64_t)i * N + j] = (float)(2 * (L - m[r][c]));
    }
  }
}

// Row i: beta from 1 with beta_min = -inf, beta_max = +inf, at most 100 steps; each step P_j = exp(-d_j beta), S = sum P_j
// (1e-8 if 0), H = log S + beta sum(d_j P_j) / S; stop when |H - log(perplexity)| <= 1e-5, else double / halve / bisect.
// beta_out / S_out: the beta and S of the last evaluation, which the conditional P_ij = exp(-d_ij beta) / S (fp32) uses.
// One 1024-thread workgroup per row; thread t holds d_j, j = t + 1024 k, in registers for k < TS_REG (j < 25600) and in LDS
// beyond (hi[j - 25600], up to 156 KB at N = 65536), so a step reads no global memory.  Sums: per thread over k ascending, a
// butterfly per wave, then the 16 wave sums in wave order.
constexpr int TS_SEARCH_THREADS = 1024;
constexpr int TS_REG = 25;  // 25 in registers + (65536 - 25600) * 4 B of LDS fits the 160 KB
constexpr int TS_REG_N = TS_REG * TS_SEARCH_THREADS;

__device__ __forceinline__ void search_term(double dj, double beta, double& s, double& sd) {
  const double p = exp(-dj * beta);
  s += p;
  sd += dj * p;
}

__global__ __launch_bounds__(TS_SEARCH_THREADS) void search_kernel(float* __restrict__ P, double* __restrict__ beta_out,
                                                                   double* __restrict__ S_out, int N, double target) {
  extern __shared__ float hi[];  // [max(N - TS_REG_N, 0)]
  __shared__ double part[2][2][TS_SEARCH_THREADS / 64];
  const int tid = threadIdx.x;
  const int i = blockIdx.x;
  float* row = P + (int64_t)i * N;
  float d[TS_REG];
#pragma unroll
  for (int k = 0; k < TS_REG; ++k) {
    const int j = tid + TS_SEARCH_THREADS * k;
    d[k] = j < N ? row[j] : 0.0f;
  }
  for (int j = TS_REG_N + tid; j < N; j += TS_SEARCH_THREADS) hi[j - TS_REG_N] = row[j];
  __syncthreads();
  const double inf = __builtin_inf();
  double beta = 1.0, bmin = -inf, bmax = inf, used = 1.0, S = 1.0;
  for (int step = 0; step < 100; ++step) {
    double v[2] = {0.0, 0.0};  // s, sd: from +0.0 and only added to, so no wave total is -0.0
#pragma unroll
    for (int k = 0; k < TS_REG; ++k) {
      const int j = tid + TS_SEARCH_THREADS * k;
      if (j < N && j != i) search_term((double)d[k], beta, v[0], v[1]);
    }
    for (int j = TS_REG_N + tid; j < N; j += TS_SEARCH_THREADS)
      if (j != i) search_term((double)hi[j - TS_REG_N], beta, v[0], v[1]);
    block_sum<kSequential, false>(v, part[step & 1]);  // alternate buffers: one barrier per step
    double s = v[0];
    const double sd = v[1];
    if (s == 0.0) s = 1e-8;
    const double H = log(s) + beta * (sd / s);
    used = beta;
    S = s;
    if (fabs(H - target) <= 1e-5) break;  // the same in every thread: the loop exits together
    if (H > target) {
      bmin = beta;
      beta = bmax == inf ? beta * 2.0 : (beta + bmax) / 2.0;
    } else {
      bmax = beta;
      beta = bmin == -inf ? beta / 2.0 : (beta + bmin) / 2.0;
    }
  }
#pragma unroll
  for (int k = 0; k < TS_REG; ++k) {
    const int j = tid + TS_SEARCH_THREADS * k;
    if (j < N) row[j] = j == i ? 0.0f : (float)(exp(-(double)d[k] * used) / S);
  }
  for (int j = TS_REG_N + tid; j < N; j += TS_SEARCH_THREADS)
    row[j] = j == i ? 0.0f : (float)(exp(-(double)hi[j - TS_REG_N] * used) / S);
  if (tid == 0) {
    beta_out[i] = used;
    S_out[i] = S;
  }
}

// P[i][j] = P[j][i] = P[i][j] + P[j][i] over the tile pair (I, J), I <= J; the diagonal tiles write once.
__global__ __launch_bounds__(256) void symmetrize_kernel(float* __restrict__ P, int N) {
  const int I = blockIdx.y, J = blockIdx.x;
  if (J < I) return;
  __shared__ float a[TS_TILE][TS_TILE + 1];  // a[r][c] = P[I0 + r][J0 + c]
  __shared__ float b[TS_TILE][TS_TILE + 1];  // b[r][c] = P[J0 + r][I0 + c]
  const int I0 = I * TS_TILE, J0 = J * TS_TILE, tid = threadIdx.x;
  for (int e = tid; e < TS_TILE * TS_TILE; e += 256) {
    const int r = e / TS_TILE, c = e % TS_TILE;
    a[r][c] = (I0 + r < N && J0 + c < N) ? P[(int64_t)(I0 + r) * N + J0 + c] : 0.0f;
    b[r][c] = (J0 + r < N && I0 + c < N) ? P[(int64_t)(J0 + r) * N + I0 + c] : 0.0f;
  }
  __syncthreads();
  for (int e = tid; e < TS_TILE * TS_TILE; e += 256) {
    const int r = e / TS_TILE, c = e % TS_TILE;
    if (I0 + r < N && J0 + c < N) P[(int64_t)(I0 + r) * N + J0 + c] = a[r][c] + b[c][r];
    if (I != J && J0 + r < N && I0 + c < N) P[(int64_t)(J0 + r) * N + I0 + c] = b[r][c] + a[c][r];
  }
}

__global__ __launch_bounds__(256) void rowsum_kernel(const float* __restrict__ P, double* __restrict__ rowsum, int N) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const float* row = P + (int64_t)i * N;
  double s = 0.0;
  for (int j = lane; j < N; j += 64)
    if (j != i) s += (double)row[j];
  s = wave_sum_lane0(s);
  if (lane == 0) rowsum[i] = s;
}

// out[0] = sum x[0..n) (sqrt of it when take_sqrt): one workgroup, thread t sums t, t + 256, ... then a fixed tree
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ x, double* __restrict__ out, int n, int take_sqrt) {
  __shared__ double part[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int k = tid; k < n; k += 256) s += x[k];
  s = tree256_sum<false>(s, part);
  if (tid == 0) out[0] = take_sqrt ? sqrt(s) : s;
}

__global__ __launch_bounds__(256) void normalize_kernel(float* __restrict__ P, const double* __restrict__ total, int N) {
  const int i = blockIdx.x;
  const double t = fmax(total[0], TS_EPS);
  float* row = P + (int64_t)i * N;
  for (int j = threadIdx.x; j < N; j += 256)
    if (j != i) row[j] = (float)fmax((double)row[j] / t, TS_EPS);
}

__global__ __launch_bounds__(256) void numsum_kernel(const double* __restrict__ Y, double* __restrict__ rowZ, int N) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const double yx = Y[2 * i], yy = Y[2 * i + 1];
  double s = 0.0;
  for (int j = lane; j < N; j += 64) {
    if (j == i) continue;
    const double dx = yx - Y[2 * j], dy = yy - Y[2 * j + 1];
    s += 1.0 / (1.0 + (dx * dx + dy * dy));
  }
  s = wave_sum_lane0(s);
  if (lane == 0) rowZ[i] = s;
}

// grad_i = 4 sum_j != i (e P_ij - Q_ij) num_ij (y_i - y_j), Q = max(num / Z, eps); KL_i = sum_j e P_ij log(max(e P_ij, eps) / Q_ij)
// when WANT_KL.  Then, per component: gains += 0.2 where update * grad < 0, else *= 0.8, clipped to >= 0.01; grad *= gains;
// update = momentum update - lr grad; y_next = y + update.  gsq[i] = |gained grad_i|^2.
template <bool WANT_KL>
__global__ __launch_bounds__(256) void grad_kernel(const float* __restrict__ P, const double* __restrict__ Y, double* __restrict__ Ynext,
                                                   double* __restrict__ update, double* __restrict__ gains, double* __restrict__ grad,
                                                   const double* __restrict__ Zp, double* __restrict__ klrow,
                                                   double* __restrict__ gsq, int N, double exag, double momentum, double lr) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const float* row = P + (int64_t)i * N;
  const double Z = Zp[0];
  const double yx = Y[2 * i], yy = Y[2 * i + 1];
  double gx = 0.0, gy = 0.0, kl = 0.0;
  for (int j = lane; j < N; j += 64) {
    if (j == i) continue;
    const double dx = yx - Y[2 * j], dy = yy - Y[2 * j + 1];
    const double num = 1.0 / (1.0 + (dx * dx + dy * dy));
    const double q = fmax(num / Z, TS_EPS);
    const double ep = exag * (double)row[j];
    const double coef = (ep - q) * num;
    gx += coef * dx;
    gy += coef * dy;
    if (WANT_KL) kl += ep * log(fmax(ep, TS_EPS) / q);
  }
  gx = wave_sum_lane0(gx);
  gy = wave_sum_lane0(gy);
  if (WANT_KL) kl = wave_sum_lane0(kl);
  if (lane != 0) return;
  const double g0[2] = {4.0 * gx, 4.0 * gy};
  const double y0[2] = {yx, yy};
  double sq = 0.0;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t k = 2 * (int64_t)i + c;
    double u = update[k], gn = gains[k], g = g0[c];
    gn = u * g < 0.0 ? gn + 0.2 : gn * 0.8;
    if (gn < 0.01) gn = 0.01;
    g *= gn;
    u = momentum * u - lr * g;
    update[k] = u;
    gains[k] = gn;
    grad[k] = g;
    Ynext[k] = y0[c] + u;
    sq += g * g;
  }
  gsq[i] = sq;
  if (WANT_KL) klrow[i] = kl;
}

}  // namespace alvq

using namespace alvq;

static int check_n(int N, const char* who) {
  ALVQ_REQUIRE(N >= 2 && N <= TS_MAX_N, ALVQ_EINVAL, "%s: N=%d outside [2, %d]", who, N, TS_MAX_N);
  return 0;
}

extern "C" int alvq_tsne_code_sqdist_f32(const int32_t* codes, float* d2, int N, int L, void* stream) {
  const char* who = "alvq_tsne_code_sqdist_f32";
  ALVQ_REQUIRE(codes && d2, ALVQ_EINVAL, "%s: null pointer", who);
  if (int rc = check_n(N, who)) return rc;
  ALVQ_REQUIRE(L >= 1 && L <= TS_MAX_L, ALVQ_EINVAL, "%s: L=%d outside [1, %d]", who, L, TS_MAX_L);
  const int T = (N + TS_TILE - 1) / TS_TILE;
  hipLaunchKernelGGL(sqdist_kernel, dim3(T, T), dim3(256), 0, (hipStream_t)stream, (const int*)codes, d2, N, L);
  return check_launch(who);
}

extern "C" int64_t alvq_tsne_affinities_workspace_bytes(int N) {
  if (N < 2 || N > TS_MAX_N) return -1;
  return ((int64_t)N + 1) * (int64_t)sizeof(double);
}

extern "C" int alvq_tsne_affinities_f32(float* P, double* beta, double* S, void* workspace, int N, double perplexity, void* stream) {
  const char* who = "alvq_tsne_affinities_f32";
  ALVQ_REQUIRE(P && beta && S && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  if (int rc = check_n(N, who)) return rc;
  ALVQ_REQUIRE(perplexity > 0.0 && perplexity < (double)N, ALVQ_EINVAL, "%s: perplexity=%g outside (0, N=%d)", who, perplexity, N);
  hipStream_t s = (hipStream_t)stream;
  double* rowsum = (double*)workspace;  // [N]
  double* total = rowsum + N;           // [1]
  const int T = (N + TS_TILE - 1) / TS_TILE, rows4 = (N + 3) / 4;
  static DeviceOnce attr;  // once per device (not inside a graph capture on every call)
  if (attr.need())
    (void)hipFuncSetAttribute((const void*)search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (TS_MAX_N - TS_REG_N) * (int)sizeof(float));
  const size_t hi_bytes = N > TS_REG_N ? (size_t)(N - TS_REG_N) * sizeof(float) : 0;
  hipLaunchKernelGGL(search_kernel, dim3(N), dim3(TS_SEARCH_THREADS), hi_bytes, s, P, beta, S, N, log(perplexity));
  hipLaunchKernelGGL(symmetrize_kernel, dim3(T, T), dim3(256), 0, s, P, N);
  hipLaunchKernelGGL(rowsum_kernel, dim3(rows4), dim3(256), 0, s, (const float*)P, rowsum, N);
  hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)rowsum, total, N, 0);
  hipLaunchKernelGGL(normalize_kernel, dim3(N), dim3(256), 0, s, P, (const double*)total, N);
  return check_launch(who);
}

extern "C" int64_t alvq_tsne_descend_workspace_bytes(int N) {
  if (N < 2 || N > TS_MAX_N) return -1;
  return (5 * (int64_t)N + 1) * (int64_t)sizeof(double);
}

extern "C" int alvq_tsne_descend_f64(const float* P, double* Y, double* update, double* gains, double* grad, double* stats,
                                     void* workspace, int N, int n_iter, double exaggeration, double momentum, double learning_rate,
                                     void* stream) {
  const char* who = "alvq_tsne_descend_f64";
  ALVQ_REQUIRE(P && Y && update && gains && grad && stats && workspace, ALVQ_EINVAL, "%s: null pointer", who);
  if (int rc = check_n(N, who)) return rc;
  ALVQ_REQUIRE(n_iter >= 1, ALVQ_EINVAL, "%s: n_iter=%d (need >= 1)", who, n_iter);
  ALVQ_REQUIRE(exaggeration > 0.0 && learning_rate > 0.0 && momentum >= 0.0 && momentum < 1.0, ALVQ_EINVAL,
               "%s: exaggeration=%g learning_rate=%g momentum=%g (need > 0, > 0, [0, 1))", who, exaggeration, learning_rate, momentum);
  hipStream_t s = (hipStream_t)stream;
  double* Y2 = (double*)workspace;  // [2N] the other ping-pong buffer
  double* rowZ = Y2 + 2 * (int64_t)N;
  double* klrow = rowZ + N;
  double* gsq = klrow + N;
  double* Z = gsq + N;  // [1]
  const int rows4 = (N + 3) / 4;
  double* cur = Y;
  double* nxt = Y2;
  for (int it = 0; it < n_iter; ++it) {
    hipLaunchKernelGGL(numsum_kernel, dim3(rows4), dim3(256), 0, s, (const double*)cur, rowZ, N);
    hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)rowZ, Z, N, 0);
    if (it == n_iter - 1)
      hipLaunchKernelGGL(grad_kernel<true>, dim3(rows4), dim3(256), 0, s, P, (const double*)cur, nxt, update, gains, grad,
                         (const double*)Z, klrow, gsq, N, exaggeration, momentum, learning_rate);
    else
      hipLaunchKernelGGL(grad_kernel<false>, dim3(rows4), dim3(256), 0, s, P, (const double*)cur, nxt, update, gains, grad,
                         (const double*)Z, klrow, gsq, N, exaggeration, momentum, learning_rate);
    double* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (cur != Y) {
    const hipError_t e = hipMemcpyAsync(Y, cur, 2 * (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, s);
    ALVQ_REQUIRE(e == hipSuccess, (int)e, "%s: %s", who, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)klrow, stats, N, 0);
  hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)gsq, stats + 1, N, 1);
  return check_launch(who);
}
