// The one owner of the vocabulary the microphone-array kernels share (included by beamform.hip, subspace.hip, herm_eig.h,
// iva_kernels.h and through it iva.hip and ilrma.hip, cacgmm.hip, wpe.hip, steered_map.h and through it srp_phat.hip,
// separation_metrics.hip, permutation_align.hip):
//   scalars      Cplx<R> (the complex type of a real type), is_finite, the complex products cmul / cmul_conj / conj_cmul, the
//                quotient cdiv, and cshfl, a double2 read from another lane.  The library is built with -ffp-contract=off, so
//                every product and sum here is rounded where it is written: a helper has the bits of its expression, and
//                moving an expression into one leaves the kernel's machine code as it was.
//   host side    capped_grid / kMaxBlocks, the dispatch over a compile-time size 1 .. 8 or 2 .. 8, and the range checks of the
//                bins, microphones and frames with the one message text the callers and tests see.
// What is not here, on purpose (the measurements: profiles/array_wave_ab.txt):
//   the lane-per-entry layout (lane 8 r + c holds entry (r, c); bf_mvdr_kernel, bf_gev_kernel, sub_eigh_kernel,
//                cac_eig_kernel, iva_solve_kernel, iva_project_kernel, herm_eig) stays two lines in each kernel.  As a value
//                type built from (lane, D) it changes the code of every one of them, and iva_solve_kernel<2> and
//                iva_project_kernel<*, 2> then take 88 VGPRs instead of 80 and 70: one wave a SIMD fewer.
//   the packed Hermitian sums of bf_cov_kernel, iva_cov_kernel and cac_cov_kernel (the weighted frame term, and lane i D + j
//                picking its entry) stay written out.  Through shared helpers, returning by value, no kernel gains registers
//                or scratch, but bf_cov_kernel<double, 8, 1> and iva_cov_kernel<double, 2> were slower on the device by more
//                than the parent's own spread.  bf_cov_kernel's frame term differs anyway: it multiplies the mask into x_i
//                first, which rounds differently and is its documented definition (include/alvq.h).
//   the three factorisations (bf_cholesky and its substitutions, iva_solve, WPE's LDS Cholesky) are different algorithms on
//                two layouts, and the status constants belong to their families.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>

#include "alvq_common.h"

namespace alvq {

// ---------------------------------------------------------------------------------------------------------------------- scalars
template <typename R> struct Cplx;
template <> struct Cplx<float> { typedef float2 type; };
template <> struct Cplx<double> { typedef double2 type; };

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= DBL_MAX; }

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {              // a b
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cmul_conj(double2 a, double2 b) {         // a conj(b); imaginary part exactly 0 for a == b
  return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ double2 conj_cmul(double2 a, double2 b) {         // conj(a) b
  return make_double2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ double2 cdiv(double2 a, double2 p) {              // a / p as a conj(p) / |p|^2
  const double den = p.x * p.x + p.y * p.y;
  return make_double2((a.x * p.x + a.y * p.y) / den, (a.y * p.x - a.x * p.y) / den);
}
__device__ __forceinline__ double2 cshfl(double2 v, int src) { return make_double2(__shfl(v.x, src, 64), __shfl(v.y, src, 64)); }

// -------------------------------------------------------------------------------------------------------------------- host side
constexpr long kMaxBlocks = 1 << 16;       // every capped grid ends here (2^24 threads, far more than the chip holds) and strides
inline dim3 capped_grid(long blocks) { return dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)); }

constexpr int kMaxMics = 8;                // a wave holds an 8 x 8 matrix, an entry a lane; sources and classes share the cap
constexpr int kMaxFrames = 65535;

// CALL(N) with the compile-time N = n; the callers have checked the range
#define ALVQ_FOR_2_TO_8(n, CALL) \
  switch (n) {                   \
    case 2: CALL(2); break;      \
    case 3: CALL(3); break;      \
    case 4: CALL(4); break;      \
    case 5: CALL(5); break;      \
    case 6: CALL(6); break;      \
    case 7: CALL(7); break;      \
    default: CALL(8); break;     \
  }
#define ALVQ_FOR_1_TO_8(n, CALL) \
  switch (n) {                   \
    case 1: CALL(1); break;      \
    case 2: CALL(2); break;      \
    case 3: CALL(3); break;      \
    case 4: CALL(4); break;      \
    case 5: CALL(5); break;      \
    case 6: CALL(6); break;      \
    case 7: CALL(7); break;      \
    default: CALL(8); break;     \
  }

inline int check_bins(const char* who, int B, int F) {
  ALVQ_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && (long)B * F <= INT_MAX, ALVQ_EINVAL,
               "%s: B=%d F=%d (need 1 <= B <= 65535, F >= 1, B F <= 2^31 - 1)", who, B, F);
  return ALVQ_OK;
}
inline int check_mics(const char* who, int D, int min_D = 1) {
  ALVQ_REQUIRE(D >= min_D && D <= kMaxMics, ALVQ_EINVAL, "%s: D=%d (need %d <= D <= 8)", who, D, min_D);
  return ALVQ_OK;
}
inline int check_frames(const char* who, int T, int min_T = 1) {
  ALVQ_REQUIRE(T >= min_T && T <= kMaxFrames, ALVQ_EINVAL, "%s: T=%d (need %d <= T <= 65535)", who, T, min_T);
  return ALVQ_OK;
}
// leaves the calling function with a check's code unless it is ALVQ_OK
#define ALVQ_TRY(check)                  \
  do {                                   \
    const int rc_ = (check);             \
    if (rc_ != ALVQ_OK) return rc_;      \
  } while (0)

}  // namespace alvq
