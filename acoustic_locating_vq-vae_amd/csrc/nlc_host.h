// Host side of the NLC (16-bit) entry points: the geometry of the padded layout, the argument checks, the kernel table that
// feeds both the LDS-limit loop and the launch, and the plan of a weight-gradient launch.  Host code only -- no kernel lives
// here, so including it adds nothing to a translation unit's device code.
//
// A new instantiation is registered by one put() in its family's table (the slot function takes the template arguments); a
// new format gets its exports from check_conv_args / check_wgrad_args / check_nlc_dims, a KernelTable and wgrad_plan (wgrad_plan_rows).
#pragma once
#include <type_traits>

#include "bf16_common.h"

namespace alvq {

// ------------------------------------------------------------------------------------------------------------------ geometry
inline int pad_to(int x, int q) { return (x + q - 1) / q * q; }
// elements of one plane of an activation: its rows and the guard rows on either side
inline long nlc_plane_elems(int B, int L, int C) {
  return ((long)alvq_nlc_rows(B, L) + 2L * alvq_nlc_guard_rows()) * pad_to(C, TB_K);
}
struct NlcDims {
  int rows, Cp;   // of the padded matrix act[rows][Cp]
  long plane;     // element offset from one plane of a multi-plane format to the next
  NlcDims(int B, int C, int L) : rows((int)alvq_nlc_rows(B, L)), Cp(pad_to(C, TB_K)), plane(nlc_plane_elems(B, L, C)) {}
  dim3 grid32() const { return dim3((rows / 32) * (Cp / 32)); }   // the 32 x 32 tiles of the layout conversions
};

// ---------------------------------------------------------------------------------------------------------- argument checks
// Each returns ALVQ_OK or the status of the first broken rule, with the message set; `who` is the export that was called.
inline int check_nlc_dims(const char* who, bool pointers, int B, int C, int L) {
  ALVQ_REQUIRE(pointers, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(B > 0 && C > 0 && L > 0, ALVQ_EINVAL, "%s: bad dims", who);
  return ALVQ_OK;
}

// ncl_also: what the fp32-NCL epilogue fuses besides the bias, in the export's own words ("" for most)
inline int check_conv_args(const char* who, const void* x, const void* wp, const void* skip1, const void* skip2, const void* mask,
                           const void* post, const void* y, const void* y2, const void* y_ncl, int B, int C, int M, int L, int KW,
                           int relu, const void* mask_bits, const void* bits_out, const char* ncl_also = "") {
  ALVQ_REQUIRE(x && wp && (y || y_ncl), ALVQ_EINVAL, "%s: null x/wp/y", who);
  ALVQ_REQUIRE(!(y && y_ncl), ALVQ_EINVAL, "%s: choose one of y (NLC) and y_ncl (NCL fp32)", who);
  ALVQ_REQUIRE(B > 0 && C > 0 && M > 0 && L > 0, ALVQ_EINVAL, "%s: bad dims", who);
  ALVQ_REQUIRE(KW == 1 || KW == 3, ALVQ_EUNSUPPORTED, "%s: KW=%d (only 1 and 3)", who, KW);
  ALVQ_REQUIRE((y2 == nullptr) == (post == nullptr), ALVQ_EINVAL, "%s: y2 and post go together", who);
  ALVQ_REQUIRE(!y_ncl || (!skip1 && !skip2 && !mask && !post && !relu), ALVQ_EUNSUPPORTED,
               "%s: the NCL fp32 epilogue fuses bias%s only", who, ncl_also);
  ALVQ_REQUIRE((long)B * (L + 1) < (1L << 30), ALVQ_EUNSUPPORTED, "%s: problem too large", who);
  ALVQ_REQUIRE(!(mask && mask_bits), ALVQ_EINVAL, "%s: pass the mask as a tensor or as bits, not both", who);
  ALVQ_REQUIRE(!y_ncl || (!mask_bits && !bits_out), ALVQ_EUNSUPPORTED, "%s: sign bits go with the NLC output", who);
  return ALVQ_OK;
}

constexpr int WGRAD_MAXSEG = 4;   // (dy, x) pairs one weight-gradient launch can sum; every family's argument block holds as many

// dy / x: the nseg segment pointers (a _multi form passes its arrays and multi = true, a single form the addresses of its
// two pointers).  dw_may_be_null: the families that can defer their split reduction (ALVQ_WGRAD_DEFER) need no dw then.
inline int check_wgrad_args(const char* who, const void* const* dy, const void* const* x, int nseg, bool multi, const void* dw,
                            const void* workspace, int B, int C, int M, int L, int KW, int w_layout, int accumulate,
                            bool dw_may_be_null) {
  ALVQ_REQUIRE(dy && x && (multi || (dy[0] && x[0])) && (dw || (dw_may_be_null && accumulate == ALVQ_WGRAD_DEFER)) && workspace,
               ALVQ_EINVAL, "%s: null pointer", who);
  if (multi) {
    ALVQ_REQUIRE(nseg >= 1 && nseg <= WGRAD_MAXSEG, ALVQ_EUNSUPPORTED, "%s: nseg=%d (1..4)", who, nseg);
    for (int i = 0; i < nseg; ++i) ALVQ_REQUIRE(dy[i] && x[i], ALVQ_EINVAL, "%s: null segment %d", who, i);
  }
  ALVQ_REQUIRE(B > 0 && C > 0 && M > 0 && L > 0, ALVQ_EINVAL, "%s: bad dims", who);
  ALVQ_REQUIRE(KW == 1 || KW == 3, ALVQ_EUNSUPPORTED, "%s: KW=%d (only 1 and 3)", who, KW);
  ALVQ_REQUIRE(w_layout == ALVQ_W_OIK || w_layout == ALVQ_W_IOK, ALVQ_EINVAL, "%s: w_layout", who);
  return ALVQ_OK;
}

// ------------------------------------------------------------------------------------------------------------ kernel tables
// The instantiations of one kernel family, each with the dynamic LDS it is launched with.  A family writes ONE constexpr slot
// function of the template arguments; its table is filled by put(slot(ARGS...), kernel<ARGS...>, lds) under for_values, and
// a launch picks launch(slot(run-time values), ...) -- so what raise_lds_limit() prepares is exactly what can be launched.
template <int... V, class F>
inline void for_values(F f) {
  (f(std::integral_constant<int, V>{}), ...);
}

template <class Fn, int N>
struct KernelTable {
  Fn fn[N] = {};
  int lds[N] = {};
  void put(int slot, Fn f, int lds_bytes) {
    fn[slot] = f;
    lds[slot] = lds_bytes;
  }
  // hipFuncSetAttribute holds for the current device only: call under a DeviceOnce
  void raise_lds_limit() const {
    for (int i = 0; i < N; ++i)
      if (fn[i]) (void)hipFuncSetAttribute((const void*)fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, lds[i]);
  }
  template <class... A>
  int launch(int slot, dim3 grid, dim3 block, hipStream_t s, const char* what, const A&... args) const {
    ALVQ_REQUIRE(slot >= 0 && slot < N && fn[slot], ALVQ_EUNSUPPORTED, "%s: no kernel is instantiated for this case (slot %d)", what,
                 slot);
    hipLaunchKernelGGL(fn[slot], grid, block, lds[slot], s, args...);
    return check_launch(what);
  }
};

// ---------------------------------------------------------------------------------------------------------- weight gradient
// Split plan of the NLC weight-gradient kernels (bf16, bf16x3, f16mx): the contraction runs over `total_rows` (a multiple
// of 64; nseg * rows for a multi-segment launch) and is cut into about 256 / tiles ranges (one workgroup per CU), at most 64.
inline int wgrad_split_plan(int total_rows, int tiles, int* chunks_per_split) {
  const int nchunks = total_rows / 64;
  int want = (256 + tiles - 1) / tiles;
  if (want < 1) want = 1;
  if (want > nchunks) want = nchunks;
  if (want > 64) want = 64;
  const int cps = (nchunks + want - 1) / want;
  *chunks_per_split = cps;
  return (nchunks + cps - 1) / cps;
}

// Largest split count any launch over 1..maxseg segments of `rows` rows can use.  ceil(n / ceil(n / want)) is NOT monotone
// in n (round-2 advisor finding: sizing for maxseg * rows alone under-sized the 3-segment launches), so take the maximum.
inline int wgrad_split_bound(int rows, int tiles, int maxseg) {
  int best = 1, cps;
  for (int s = 1; s <= maxseg; ++s) {
    const int k = wgrad_split_plan(s * rows, tiles, &cps);
    if (k > best) best = k;
  }
  return best;
}

// the (m, c) tile a weight-gradient workgroup owns, all taps of it
struct WgradTile {
  int mt, ct;
  int count(int C, int M) const { return ((M + mt - 1) / mt) * ((C + ct - 1) / ct); }
};

inline bool wgrad_shape_ok(int B, int C, int M, int L, int KW) { return B > 0 && C > 0 && M > 0 && L > 0 && (KW == 1 || KW == 3); }

// behind *_workspace_bytes of the two-plane formats: the split partials, then bias_splits * pad64(M) floats of bias partials
inline int64_t wgrad_workspace_bytes(int B, int C, int M, int L, int KW, WgradTile t, int bias_splits) {
  if (!wgrad_shape_ok(B, C, M, L, KW)) return -1;
  const int splits = wgrad_split_bound((int)alvq_nlc_rows(B, L), t.count(C, M), WGRAD_MAXSEG);
  return (int64_t)splits * KW * M * C * 4 + (int64_t)bias_splits * pad_to(M, 64) * 4;
}
// behind *_splits: the split count a launch of nseg segments uses
inline int wgrad_splits(int B, int C, int M, int L, int KW, int nseg, WgradTile t) {
  if (!wgrad_shape_ok(B, C, M, L, KW) || nseg < 1 || nseg > WGRAD_MAXSEG) return -1;
  int cps;
  return wgrad_split_plan(nseg * (int)alvq_nlc_rows(B, L), t.count(C, M), &cps);
}

// Fills what every family's argument block (WgradV2Args, WgradX3Args, WgradFxArgs; zero-initialised by the caller) holds:
// segments, tiles and the split plan over nseg segments of `rows` rows, which it holds to the bound `family`_workspace_bytes
// sizes for tile t.  The launch, the split reduction and the bias reduction are the caller's.
template <class Args>
inline int wgrad_plan_rows(const char* family, Args& a, const void* const* dy, const void* const* x, int nseg, void* workspace,
                           int rows, int C, int M, WgradTile t) {
  static_assert(sizeof(a.dy) / sizeof(a.dy[0]) == WGRAD_MAXSEG && sizeof(a.x) == sizeof(a.dy), "segment count of the family");
  for (int i = 0; i < WGRAD_MAXSEG; ++i) {
    a.dy[i] = (const u16*)dy[i < nseg ? i : 0];
    a.x[i] = (const u16*)x[i < nseg ? i : 0];
  }
  a.nseg = nseg;
  a.partial = (float*)workspace;
  a.Mp = pad_to(M, 64); a.Cp = pad_to(C, 64); a.M = M; a.C = C;
  a.mtiles = (M + t.mt - 1) / t.mt; a.ctiles = (C + t.ct - 1) / t.ct;
  a.total_rows = rows;
  a.splits = wgrad_split_plan(nseg * rows, a.mtiles * a.ctiles, &a.chunks_per_split);
  ALVQ_REQUIRE(a.splits <= wgrad_split_bound(rows, t.count(C, M), WGRAD_MAXSEG), ALVQ_EINVAL,
               "%s: %d splits exceed what %s_workspace_bytes sizes", family, a.splits, family);
  return ALVQ_OK;
}

// The two-plane formats on top of it: the plane offsets too.  *bias_partial: where the bias partials start in the workspace.
template <class Args>
inline int wgrad_plan(const char* family, Args& a, const void* const* dy, const void* const* x, int nseg, void* workspace, int B,
                      int C, int M, int L, int KW, WgradTile t, float** bias_partial) {
  if (int rc = wgrad_plan_rows(family, a, dy, x, nseg, workspace, (int)alvq_nlc_rows(B, L), C, M, t)) return rc;
  a.dy_plane = nlc_plane_elems(B, L, M);
  a.x_plane = nlc_plane_elems(B, L, C);
  *bias_partial = (float*)((char*)workspace + (int64_t)a.splits * KW * M * C * 4);
  return ALVQ_OK;
}

}  // namespace alvq
