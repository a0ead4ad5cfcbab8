// f16mx weight gradient (format: f16mx_common.h):
//
//   dW_t[m][c] = sum_rows dY[row][m] * X[row + t - pad][c]        (all taps t of one (m, c) tile per workgroup)
//
// Same decomposition, staging and split reduction as the bf16x3 weight gradient (conv1d_bf16x3.hip): workgroup = 128 m x
// CT c x all taps, 8 waves (2 along m x 4 along c), K-tile = 32 rows = a dY slab pair and an X slab pair (H and Q planes)
// in one of two LDS stages.  The contraction runs over ROWS, the slow axis of both operands, so fragments come from the
// transposing LDS reads: ds_read_b64_tr_b16 for the fp16 planes, ds_read_b64_tr_b8 for the fp8 planes.  A wave's block
// is 2 (m) x NC (c) x KW tiles of 32x32 and a K-tile is two phases -- fp16 main term (2 k-steps of 32x32x16), barrier,
// fp8 cross terms (one block-scaled 32x32x64 per tile: block 0 = dY.hi8 x X.lo8, block 1 = dY.lo8 x X.hi8) -- with the
// other phase's fragments and the next K-tile's DMA in flight meanwhile.  A loss scale carried by dY is divided out
// (exactly: it is a power of two) when the fp32 partials are written.  The bias gradient (column sums of dY) is a
// separate bandwidth-bound pass here: as all-ones products in this kernel it needs two more 32x32 accumulators (32
// VGPRs), which the KW = 3 instantiation does not have.
#include <stdlib.h>

#include "alvq_common.h"
#include "f16mx_common.h"
#include "nlc_host.h"
#include "wgrad_reduce.h"
#include "wgrad_tile.h"

namespace alvq {

struct WgradFxArgs {
  // Up to WGRAD_MAXSEG (dy, x) pairs of identical shape whose products are summed into ONE dW: the R uses of a shared
  // residual weight (residual_stack.py:40-41) become a single longer contraction -- one split reduction instead of R.
  // Rows are numbered through all segments: virtual row v = seg * total_rows + r (total_rows % 64 == 0, so neither a
  // 64-row chunk nor a 32-row K-tile straddles two segments).
  const u16* dy[WGRAD_MAXSEG];
  const u16* x[WGRAD_MAXSEG];
  int nseg;
  float* partial;        // [splits][KW][M][C]
  const float* inv_scale;   // device scalar multiplied into every partial (1 / loss scale), or null
  long dy_plane, x_plane;
  int Mp, Cp, M, C;
  int mtiles, ctiles, splits, chunks_per_split, total_rows;
  int e;                 // E8M0 scale exponent of both operands (activations / scaled gradients)
  int dbg;               // ablation switches of the DBG instantiation (ALVQ_FX_DBG, as in conv1d_f16mx.hip): 1, 2, 4, 8
};

// NC / MF = 32-wide tiles per wave along c / along m: (1, 2) for KW = 3 (workgroup tile 128 m x 128 c x 3 taps, 96
// accumulator VGPRs) and (2, 4) for KW = 1 (256 m x 256 c, 128 accumulator VGPRs: the convolution's tile, at which a
// K-tile moves 32 bytes per matrix-pipe cycle per CU through LDS-DMA; the 128 x 256 tile of the first version moved 47).
template <int KW, int NC, int MF, bool DBG = false>
__global__ __launch_bounds__(512, 2) void conv1d_wgrad_f16mx_kernel(WgradFxArgs a) {
  const int dbg = DBG ? a.dbg : 0;
  constexpr int MT = 2 * MF * 32, CT = 4 * NC * 32;
  // a stage: dY.H, dY.Q, X.H, X.Q (the Q plane has a bf16 plane's geometry: 64 bytes per 32 channels)
  typedef WgradSlabs<KW, MT, CT, 2> Slabs;
  constexpr int YRB = Slabs::YRB, XRB = Slabs::XRB, YBYTES = Slabs::YBYTES, XBYTES = Slabs::XBYTES, STAGE = Slabs::STAGE;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave >> 2) * (MF * 32), wc0 = (wave & 3) * NC * 32;
  const WgradWork w = wgrad_work<MT, CT>(a);
  const int n = w.n;
  WgradStager<WgradFxArgs, KW, MT, CT, 2, LdsDmaAsm> st(a, wave, lane, w);

  // ---- transposed fragment reads.  Lane l: i = l & 15 (lane of its 16-group), blk = (l >> 4) & 1 (which 16-column half
  // of the 32-wide tile), g = l >> 5 (k group of the MFMA).
  //  fp16 (tr_b16: a 16-group reads a 4-row x 16-column block; lane 4q+p supplies the address of block row q, columns
  //    4p..4p+3 -- ANY LDS row may stand for block row q):  k-step s, group g covers the 8 rows 2q + g + 8s (first
  //    read) and 16 + 2q + g + 8s (second read), q = 0..3 -- the same permutation of the K-tile's rows for both operands,
  //    which a contraction does not care about.  A half-wave (one g) holds two 16-column blocks, i.e. two neighbouring
  //    32-byte segments L and L+1, times four rows: with rows of ONE parity the (row & 7) segment swizzle sends the
  //    block-0 lanes to L ^ {g, 2+g, 4+g, 6+g} and the block-1 lanes to the complementary four segments -- 8 distinct
  //    segments, conflict-free for every tap offset (four CONSECUTIVE rows collide two-fold: measured 33 % of the
  //    LDS cycles in this kernel).
  //  fp8 (tr_b8: an 8-row x 16-column block; lane 2q+p supplies row q, bytes 8p..8p+7): group g covers rows 16g..16g+15
  //    in two reads, once in the hi8 segment and once in the lo8 segment of the tile's 64-byte chunk.
  const int i16 = lane & 15, blk = (lane >> 4) & 1, g = lane >> 5;
  const int qrow = 16 * g + (i16 >> 1);              // + 8 for the second read
  const int qbyte = 16 * blk + 8 * (i16 & 1);
  typedef int i32x2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) i32x2* lds_tr8_ptr;
  // H bases: wgrad_frag32_base (wgrad_tile.h).  Q plane, same factoring: byte offset of (row, 32-byte segment seg) in a slab
  // with ROWB-byte rows = row * ROWB + (seg >> 3) * 256 + (((seg & 7) ^ (row & 7)) << 5); fragment f at LANE BASE ^ (f << 6)
  // (^ 32 for the lo8 segment).
  const int sA = wm0 >> 4, sB = wc0 >> 4;            // first 16-column block (= 32-byte H segment) of the wave
  const int aHb = wgrad_frag32_base<YRB>(i16, blk, g, wm0, 0);
  const int aQb = qrow * YRB + qbyte + (sA >> 3) * 256 + (((sA & 7) ^ (qrow & 7)) << 5);   // Q chunk c = segments 2c, 2c+1
  int bHb[KW], bQb[KW];
#pragma unroll
  for (int t = 0; t < KW; ++t) {
    bHb[t] = wgrad_frag32_base<XRB>(i16, blk, g, wc0, t);
    bQb[t] = (qrow + t) * XRB + qbyte + (sB >> 3) * 256 + (((sB & 7) ^ ((qrow + t) & 7)) << 5);
  }

  f16x8_t aH[MF][2], bH[KW][NC][2];
  i32x8 aQ[MF], bQ[KW][NC];
  // FIRST / SECOND: byte offsets of the two 16-row column pieces that form blocks 0 and 1 of the scaled MFMA's operand
#define WF_TR8(DST, FIRST, SECOND, ROWB)                                                                         \
  {                                                                                                              \
    const i32x2 a0_ = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_tr8_ptr)(lds + (FIRST)));                     \
    const i32x2 a1_ = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_tr8_ptr)(lds + (FIRST) + 8 * (ROWB)));       \
    const i32x2 b0_ = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_tr8_ptr)(lds + (SECOND)));                    \
    const i32x2 b1_ = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_tr8_ptr)(lds + (SECOND) + 8 * (ROWB)));      \
    DST = i32x8{a0_[0], a0_[1], a1_[0], a1_[1], b0_[0], b0_[1], b1_[0], b1_[1]};                                \
  }
  // A operand (dY), tile MI; B operand (X), tap TP, tile CF: rows shifted by TP; B's blocks are (lo8, hi8) so that block 0
  // pairs dY.hi8 with X.lo8
#define WF_RDH_A(STAGE_, MI, KS) \
  aH[MI][KS] = wgrad_tr16_pair<f16x8_t>(lds + ((STAGE_) * STAGE + (aHb ^ ((MI) << 6)) + 8 * (KS) * YRB), YRB);
#define WF_RDQ_A(STAGE_, MI) \
  WF_TR8(aQ[MI], (STAGE_) * STAGE + YBYTES + (aQb ^ ((MI) << 6)), (STAGE_) * STAGE + YBYTES + (aQb ^ ((MI) << 6) ^ 32), YRB)
#define WF_RDH_B(STAGE_, TP, CF, KS) \
  bH[TP][CF][KS] = wgrad_tr16_pair<f16x8_t>(lds + ((STAGE_) * STAGE + 2 * YBYTES + (bHb[TP] ^ ((CF) << 6)) + 8 * (KS) * XRB), XRB);
#define WF_RDQ_B(STAGE_, TP, CF)                                                                 \
  WF_TR8(bQ[TP][CF], (STAGE_) * STAGE + 2 * YBYTES + XBYTES + (bQb[TP] ^ ((CF) << 6) ^ 32),      \
         (STAGE_) * STAGE + 2 * YBYTES + XBYTES + (bQb[TP] ^ ((CF) << 6)), XRB)

  // block scales: both operands are activation-class; A blocks = (hi8, lo8), B blocks = (lo8, hi8)
  int sa = g ? a.e - FX_LO_SHIFT : a.e, sb = g ? a.e : a.e - FX_LO_SHIFT;
  asm volatile("" : "+v"(sa), "+v"(sb));   // opaque: see the convolution kernel

  f32x16 acc[KW][MF][NC];
#pragma unroll
  for (int t = 0; t < KW; ++t)
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
      for (int jn = 0; jn < NC; ++jn)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][i][jn][q] = 0.f;
#define WF_MMH(MI, KS)                                                                                           \
  _Pragma("unroll") for (int tp = 0; tp < KW; ++tp) _Pragma("unroll") for (int cf = 0; cf < NC; ++cf)            \
      asm("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc[tp][MI][cf]) : "v"(aH[MI][KS]), "v"(bH[tp][cf][KS]));
#define WF_MMQ(MI)                                                                                               \
  _Pragma("unroll") for (int tp = 0; tp < KW; ++tp) _Pragma("unroll") for (int cf = 0; cf < NC; ++cf)            \
      asm("v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"                           \
          : "+v"(acc[tp][MI][cf]) : "v"(aQ[MI]), "v"(bQ[tp][cf]), "v"(sa), "v"(sb));
#define WF_SB __builtin_amdgcn_sched_barrier(0);
#define WF_ALL_B(M_) _Pragma("unroll") for (int tp = 0; tp < KW; ++tp) _Pragma("unroll") for (int cf = 0; cf < NC; ++cf) { M_ }

  // one K-tile in stage S
#define WF_ALL_A(M_) _Pragma("unroll") for (int mi = 0; mi < MF; ++mi) { M_ }
#define WF_TILE(S, MORE)                                                                                           \
  /* phase 1: fp16 main term; meanwhile this K-tile's Q fragments */                                            \
  WF_MMH(0, 0) WF_SB                                                                                             \
  if (!(dbg & 2)) { WF_ALL_B(WF_RDQ_B(S, tp, cf)) } WF_SB                                                        \
  WF_MMH(1, 0) WF_SB                                                                                             \
  if (!(dbg & 2)) { WF_ALL_A(WF_RDQ_A(S, mi)) } WF_SB                                                            \
  _Pragma("unroll") for (int mi = 2; mi < MF; ++mi) { WF_MMH(mi, 0) }                                            \
  WF_ALL_A(WF_MMH(mi, 1)) WF_SB                                                                                  \
  if (!(dbg & 4)) {                                                                                              \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                  \
    __builtin_amdgcn_s_barrier();                                                                                \
  }                                                                                                              \
  /* phase 2: fp8 cross terms; meanwhile the DMA of K-tile t+2 into this stage and the next tile's H fragments */ \
  if ((MORE) && !(dbg & 1)) st.issue(lds, S);                                                                    \
  WF_MMQ(0) WF_SB                                                                                                \
  if (!(dbg & 2)) { WF_ALL_A(WF_RDH_A((S) ^ 1, mi, 0)) WF_ALL_B(WF_RDH_B((S) ^ 1, tp, cf, 0)) } WF_SB            \
  WF_MMQ(1) WF_SB                                                                                                \
  if (!(dbg & 2)) { WF_ALL_A(WF_RDH_A((S) ^ 1, mi, 1)) WF_ALL_B(WF_RDH_B((S) ^ 1, tp, cf, 1)) } WF_SB            \
  _Pragma("unroll") for (int mi = 2; mi < MF; ++mi) { WF_MMQ(mi) }                                               \
  WF_SB

  if (n > 0) {
    st.issue(lds, 0);
    if (n > 1) st.issue(lds, 1);
    st.wait_keep(n > 1 ? 1 : 0);   // K-tile 0 landed; K-tile 1's pieces (this wave's count) may stay in flight
    __builtin_amdgcn_s_barrier();
    WF_ALL_A(WF_RDH_A(0, mi, 0) WF_RDH_A(0, mi, 1))
    WF_ALL_B(WF_RDH_B(0, tp, cf, 0) WF_RDH_B(0, tp, cf, 1))
    for (int t = 0; t < n; t += 2) {
      WF_TILE(0, t + 2 < n)
      WF_TILE(1, t + 3 < n)
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // MFMA-result -> VALU-read wait states (asm MFMAs are invisible)
  }
#undef WF_TILE
#undef WF_ALL_A
#undef WF_ALL_B
#undef WF_SB
#undef WF_MMQ
#undef WF_MMH
#undef WF_RDQ_B
#undef WF_RDH_B
#undef WF_RDQ_A
#undef WF_RDH_A
#undef WF_TR8

  // ---- partial[split][t][m][c] = acc / loss scale (fp32)
  if (dbg & 8) {
    if (acc[0][0][0][0] == 12345.678f) a.partial[0] = 1.f;
    return;
  }
  wgrad_store32<true, KW, MF, NC>(a, w, lane, g, wm0, wc0, acc, a.inv_scale ? *a.inv_scale : 1.f);
}

// ---------------------------------------------------------------------------------------------------- bias gradient
// partial[split][m] = sum over the split's rows of dY[row][m] = H + lo8 * S_lo: 64 channels x one row range per
// workgroup; thread = (8 channels, row lane of 32), rows strided by 32, then a fixed-order reduction over the row lanes.
__global__ __launch_bounds__(256) void bias_grad_fx_partial_kernel(const u16* dy, long plane, float* partial, int rows, int Mp,
                                                                   int rows_per_split, int e) {
  const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c = blockIdx.x * 64 + cg * 8;
  const int rb = blockIdx.y * rows_per_split, re = min(rows, rb + rows_per_split);
  const float s_lo = fx_pow2(e - FX_LO_SHIFT);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = rb + rl; r < re; r += 32) {
    const u32x4 h = *(const u32x4*)(dy + (long)r * Mp + c);
    const u32x2 ql = *(const u32x2*)((const unsigned char*)(dy + plane) + (long)r * Mp * 2 + fx_q_off(c) + 32);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v0, v1;
      fx_join2(h[k], ql[k >> 1], (k & 1) * 2, s_lo, v0, v1);
      s[2 * k] += v0;
      s[2 * k + 1] += v1;
    }
  }
  __shared__ float red[32][65];
#pragma unroll
  for (int k = 0; k < 8; ++k) red[rl][cg * 8 + k] = s[k];
  __syncthreads();
  if (threadIdx.x < 64) {
    float t = 0.f;
    for (int k = 0; k < 32; ++k) t += red[k][threadIdx.x];
    partial[(long)blockIdx.y * Mp + blockIdx.x * 64 + threadIdx.x] = t;
  }
}

// dbias[m] (+)= inv_scale * sum_s partial[s][m]: 32 channels x 8 split phases per workgroup (coalesced along m, 8-way
// parallel along the splits), fixed order.  The split count is a compile-time constant so that a thread's 16 loads are
// all in flight at once (as a run-time loop they were 16 round trips to L2 one after the other: 31 us for 512 KB).
constexpr int FX_BIAS_SPLITS = 128;
static __global__ __launch_bounds__(256) void wgrad_fx_bias_reduce_kernel(const float* bp, float* dbias, int Mp, int M,
                                                                          int accumulate, const float* inv_scale) {
  const int mi = threadIdx.x & 31, ph = threadIdx.x >> 5;
  const int m = blockIdx.x * 32 + mi;
  float v[FX_BIAS_SPLITS / 8];
#pragma unroll
  for (int k = 0; k < FX_BIAS_SPLITS / 8; ++k) v[k] = m < M ? bp[(long)(ph + 8 * k) * Mp + m] : 0.f;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < FX_BIAS_SPLITS / 8; ++k) s += v[k];
  __shared__ float red[8][32];
  red[ph][mi] = s;
  __syncthreads();
  if (ph == 0 && m < M) {
    float t = ((red[0][mi] + red[1][mi]) + (red[2][mi] + red[3][mi])) + ((red[4][mi] + red[5][mi]) + (red[6][mi] + red[7][mi]));
    t *= inv_scale ? *inv_scale : 1.f;
    dbias[m] = accumulate ? dbias[m] + t : t;
  }
}

template <int KW, int NC, int MF>
static constexpr int wgrad_fx_lds() {
  return 2 * WgradSlabs<KW, 2 * MF * 32, 4 * NC * 32, 2>::STAGE;
}

// tile of a launch: 128 x 128 x 3 taps for width 3, 256 x 256 for width 1
static WgradTile wgrad_fx_tile(int KW) { return KW == 3 ? WgradTile{128, 128} : WgradTile{256, 256}; }

}  // namespace alvq

using namespace alvq;

extern "C" int64_t alvq_conv1d_wgrad_f16mx_workspace_bytes(int B, int C, int M, int L, int KW) {
  return wgrad_workspace_bytes(B, C, M, L, KW, wgrad_fx_tile(KW), FX_BIAS_SPLITS);
}

extern "C" int alvq_conv1d_wgrad_f16mx_splits(int B, int C, int M, int L, int KW, int nseg) {
  return wgrad_splits(B, C, M, L, KW, nseg, wgrad_fx_tile(KW));
}

// the weight gradient behind alvq_conv1d_wgrad_f16mx and its _multi form (no bias gradient there: dbias null)
static int wgrad_fx(const char* who, const void* const* dy, const void* const* x, int nseg, bool multi, float* dw, float* dbias,
                    void* workspace, int B, int C, int M, int L, int KW, int w_layout, int accumulate, const float* inv_scale,
                    hipStream_t s) {
  if (int rc = check_wgrad_args(who, dy, x, nseg, multi, dw, workspace, B, C, M, L, KW, w_layout, accumulate, false)) return rc;
  WgradFxArgs a{};
  float* bpart;
  if (int rc = wgrad_plan("alvq_conv1d_wgrad_f16mx", a, dy, x, nseg, workspace, B, C, M, L, KW, wgrad_fx_tile(KW), &bpart)) return rc;
  a.inv_scale = inv_scale;
  a.e = FX_E_ACT;
#ifdef ALVQ_DEBUG_KERNELS   // ablation instantiations: debug library only (build.py --debug-kernels)
  static const int dbg_env = getenv("ALVQ_FX_DBG") ? atoi(getenv("ALVQ_FX_DBG")) : 0;   // timing ablations (results are garbage)
#else
  constexpr int dbg_env = 0;
#endif
  a.dbg = dbg_env;
  // conv1d_wgrad_f16mx_kernel<KW, NC, MF, DBG> sits at [DBG][KW == 3]
  static const auto table = [] {
    KernelTable<void (*)(WgradFxArgs), 4> t;
    for_values<1, 3>([&](auto kw) {
      constexpr int NC = kw == 3 ? 1 : 2, MF = kw == 3 ? 2 : 4;
      t.put(kw == 3, conv1d_wgrad_f16mx_kernel<kw, NC, MF>, wgrad_fx_lds<kw, NC, MF>());
#ifdef ALVQ_DEBUG_KERNELS
      t.put(2 + (kw == 3), conv1d_wgrad_f16mx_kernel<kw, NC, MF, true>, wgrad_fx_lds<kw, NC, MF>());
#endif
    });
    return t;
  }();
  static DeviceOnce attr;
  if (attr.need()) table.raise_lds_limit();
  if (int rc = table.launch((dbg_env ? 2 : 0) + (KW == 3), dim3(a.mtiles * a.ctiles * a.splits), dim3(512), s, "alvq_conv1d_wgrad_f16mx", a))
    return rc;
  wgrad_reduce_launch((const float*)workspace, dw, a.splits, KW, M, C, w_layout, accumulate, s);
  if (dbias) {     // single segment only (the shared residual weights have no bias)
    const int rows = a.total_rows, rps = (rows + FX_BIAS_SPLITS - 1) / FX_BIAS_SPLITS;
    hipLaunchKernelGGL(bias_grad_fx_partial_kernel, dim3(a.Mp / 64, FX_BIAS_SPLITS), dim3(256), 0, s, (const u16*)dy[0], a.dy_plane, bpart,
                       rows, a.Mp, rps, a.e);
    hipLaunchKernelGGL(wgrad_fx_bias_reduce_kernel, dim3((M + 31) / 32), dim3(256), 0, s, (const float*)bpart, dbias, a.Mp, M,
                       accumulate, inv_scale);
  }
  return check_launch("alvq_conv1d_wgrad_f16mx/reduce");
}

extern "C" int alvq_conv1d_wgrad_f16mx(const void* dy, const void* x, float* dw, float* dbias, void* workspace, int B, int C, int M,
                                       int L, int KW, int w_layout, int accumulate, const float* inv_scale, void* stream) {
  return wgrad_fx("alvq_conv1d_wgrad_f16mx", &dy, &x, 1, false, dw, dbias, workspace, B, C, M, L, KW, w_layout, accumulate, inv_scale,
                  (hipStream_t)stream);
}

extern "C" int alvq_conv1d_wgrad_f16mx_multi(const void* const* dy, const void* const* x, int nseg, float* dw, void* workspace,
                                             int B, int C, int M, int L, int KW, int w_layout, int accumulate,
                                             const float* inv_scale, void* stream) {
  return wgrad_fx("alvq_conv1d_wgrad_f16mx_multi", dy, x, nseg, true, dw, nullptr, workspace, B, C, M, L, KW, w_layout, accumulate,
                  inv_scale, (hipStream_t)stream);
}
