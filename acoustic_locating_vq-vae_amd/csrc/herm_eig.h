// Eigendecomposition of a complex Hermitian matrix of order 1 .. 8 by one wave: cyclic Jacobi in float64.  The definition is
// the comment on alvq_eigh_f64 in include/alvq.h; tests/helpers/subspace_ref.py restates it in numpy.  Used by
// sub_eigh_kernel (csrc/subspace.hip) and bf_gev_kernel (csrc/beamform.hip).
//
// Layout: the one bf_mvdr_kernel holds Phi in.  Lane 8 r + c holds entry (r, c) of A and of V; rows and columns travel by
// __shfl (ds_bpermute), no LDS and no barrier.  Both triangles are kept and updated, so that a row or a column is one shuffle
// away from the lane that needs it; every decision (the rotation's angle, whether to rotate) is taken from the lower triangle
// and the diagonal, by every lane of the two rows it concerns from the same three values: the same bits.
// Order: round robin.  With m = D rounded up to even, step s = 0 .. m - 2 pairs index m - 1 with s and every other i with
// (2 s - i) mod (m - 1): m / 2 disjoint pairs, which rotate together (a pair with an index >= D is a bye).  m - 1 steps are a
// sweep: every pair once.
// A rotation of the pair p < q with g = a_pq, |g| > 0.5 u ||A||_F / D:  zeta = (a_qq - a_pp) / (2 |g|),
// t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), cs = 1 / sqrt(1 + t^2), sn = cs t g / |g|;  J = [[cs, sn], [-conj(sn), cs]].
// A <- A J (one shuffle: the partner column), then A <- J^H A (one more: the partner row), V <- V J; then a_pq = a_qp = 0,
// a_pp -= t |g|, a_qq += t |g| are set outright, so the diagonal stays real.  A step shuffles four doubles for its angles and,
// where any of its pairs rotates (a wave-uniform test), nine more for the columns and rows; every lane of a row computes its
// pair's angle (a hypot, three divisions, two square roots), which is most of the step: the kernel is bound by float64
// issue at the vector rate, not by the shuffles.  v_mfma_f64 is not used, for the reason csrc/wpe.hip gives.
#pragma once
#include <cfloat>

#include "array_wave.h"

namespace alvq {

constexpr int HE_MAX_SWEEPS = 16;
constexpr double HE_U = 1.1102230246251565e-16;      // 2^-53
constexpr int HE_BAD_INPUT = 1;                      // a non-finite entry was read
constexpr int HE_NO_CONVERGENCE = 2;                 // HE_MAX_SWEEPS sweeps, each with a rotation

struct HermEig {
  double lam;        // the eigenvalue of the lane's column c (as Jacobi left it on the diagonal)
  int rank;          // its place in ascending order: column c of V belongs at column `rank` of the output
  int status;        // the same in every lane
};

// whom index i meets at step s of the round robin of m players (m even); an index beyond the table meets itself
__device__ __forceinline__ int he_partner(int i, int s, int m) {
  const int n = m - 1;
  if (i >= n) return i == n ? s : i;
  int j = (2 * s - i) % n;
  if (j < 0) j += n;
  return j == i ? n : j;
}

// a: entry (r, c) of the Hermitian matrix, both triangles filled from the lower one, the diagonal real, 0 outside D x D.
// On return v is entry (r, c) of V with the phase rule applied, columns still in Jacobi's order.  The whole wave calls it.
__device__ __forceinline__ HermEig herm_eig(double2 a, double2& v, int D, int lane) {
  const int r = lane >> 3, c = lane & 7;
  const bool in = r < D && c < D;
  HermEig out;
  out.status = 0;
  if (__any(in && (!is_finite(a.x) || !is_finite(a.y)))) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    v = make_double2(nan, nan);
    out.lam = nan;
    out.rank = c;
    out.status = HE_BAD_INPUT;
    return out;
  }
  v = make_double2(in && r == c ? 1.0 : 0.0, 0.0);

  // ||A||_F = mx sqrt(sum |a / mx|^2): no overflow, no underflow; both reductions are butterflies, every lane gets the result
  const double mx = wave_max(in ? fmax(fabs(a.x), fabs(a.y)) : 0.0);
  if (mx > 0.0 && D > 1) {
    const double sx = a.x / mx, sy = a.y / mx;
    const double nf = mx * sqrt(wave_sum(sx * sx + sy * sy));
    const double thr = 0.5 * HE_U * nf / (double)D;
    const int m = (D + 1) & ~1;
    out.status = HE_NO_CONVERGENCE;
    for (int sweep = 0; sweep < HE_MAX_SWEEPS; ++sweep) {
      bool rotated = false;
      for (int s = 0; s < m - 1; ++s) {
        const int pr = he_partner(r, s, m), pc = he_partner(c, s, m);
        // the pair of the lane's row: p = lo < q = hi
        const bool pair = r < D && pr < D && pr != r;
        const int lo = pair ? min(r, pr) : r, hi = pair ? max(r, pr) : r;
        const double alpha = __shfl(a.x, 9 * lo, 64), beta = __shfl(a.x, 9 * hi, 64);
        const double2 g = cshfl(a, 8 * hi + lo);                         // a_qp; a_pq is its conjugate
        const double absg = hypot(g.x, g.y);
        const bool rot = pair && absg > thr;
        double cs = 1.0, h = 0.0;
        double2 sn = make_double2(0.0, 0.0);
        if (rot) {
          const double zeta = (beta - alpha) / (2.0 * absg);
          const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          cs = 1.0 / sqrt(1.0 + t * t);
          const double sv = cs * t;
          sn = make_double2(sv * (g.x / absg), -(sv * (g.y / absg)));      // cs t a_pq / |a_pq|
          h = t * absg;
        }
        if (!__any(rot)) continue;                                         // no pair of this step rotates: nothing moves
        rotated = true;
        // the pair of the lane's column: what the lanes of row c have just computed
        const double ccs = __shfl(cs, 9 * c, 64);
        const double2 csn = cshfl(sn, 9 * c);
        const int crot = __shfl((int)rot, 9 * c, 64);
        // A <- A J, V <- V J:  col_p <- cs col_p - conj(sn) col_q,  col_q <- sn col_p + cs col_q
        const double2 ya = cshfl(a, 8 * r + pc), yv = cshfl(v, 8 * r + pc);
        if (crot) {
          if (c < pc) {
            a = make_double2(ccs * a.x - (csn.x * ya.x + csn.y * ya.y), ccs * a.y - (csn.x * ya.y - csn.y * ya.x));
            v = make_double2(ccs * v.x - (csn.x * yv.x + csn.y * yv.y), ccs * v.y - (csn.x * yv.y - csn.y * yv.x));
          } else {
            a = make_double2((csn.x * ya.x - csn.y * ya.y) + ccs * a.x, (csn.x * ya.y + csn.y * ya.x) + ccs * a.y);
            v = make_double2((csn.x * yv.x - csn.y * yv.y) + ccs * v.x, (csn.x * yv.y + csn.y * yv.x) + ccs * v.y);
          }
        }
        // A <- J^H A:  row_p <- cs row_p - sn row_q,  row_q <- conj(sn) row_p + cs row_q
        const double2 yr = cshfl(a, 8 * pr + c);
        if (rot) {
          if (r < pr)
            a = make_double2(cs * a.x - (sn.x * yr.x - sn.y * yr.y), cs * a.y - (sn.x * yr.y + sn.y * yr.x));
          else
            a = make_double2((sn.x * yr.x + sn.y * yr.y) + cs * a.x, (sn.x * yr.y - sn.y * yr.x) + cs * a.y);
          if (c == pr) a = make_double2(0.0, 0.0);
          if (c == r) a = make_double2(r < pr ? alpha - h : beta + h, 0.0);
        }
      }
      if (!rotated) {                                                      // the same in every lane
        out.status = 0;
        break;
      }
    }
  }

  // ascending order: the place of column c is the number of eigenvalues below its own, an equal one at a lower index included
  const double lam = __shfl(a.x, 9 * c, 64);
  int rank = 0;
  for (int j = 0; j < D; ++j) {
    const double lj = __shfl(a.x, 9 * j, 64);
    if (lj < lam || (lj == lam && j < c)) ++rank;
  }
  out.lam = lam;
  out.rank = rank;
  // the phase: the column's component of the largest re^2 + im^2 (the lowest index on ties) becomes real and positive
  double best = -1.0;
  double2 vm = make_double2(1.0, 0.0);
  for (int i = 0; i < D; ++i) {
    const double2 x = cshfl(v, 8 * i + c);
    const double m2 = x.x * x.x + x.y * x.y;
    if (m2 > best) {
      best = m2;
      vm = x;
    }
  }
  if (in) {
    const double hm = hypot(vm.x, vm.y);
    v = make_double2((v.x * vm.x + v.y * vm.y) / hm, (v.y * vm.x - v.x * vm.y) / hm);       // v conj(vm) / |vm|
  }
  return out;
}

}  // namespace alvq
