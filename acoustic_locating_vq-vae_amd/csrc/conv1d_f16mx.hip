// f16mx convolution (see f16mx_common.h for the format): forward / data-gradient / ConvTranspose of the wide and narrow
// layers alike, plus the boundary conversions of the format.
//
// Tiling is that of conv1d_bf16x3.hip -- 256 out-channels x 256 rows per workgroup, 8 waves, a wave owns 128 x 64;
// K-tile = (32 channels, one tap) -- with the two LDS-DMA rings of conv_tile.h (ConvRings: W.H, W.Q per K-tile; X.H, X.Q
// per chunk, shared by the taps).  The wave's block is 4 x 2 tiles of 32x32 and a K-tile is TWO phases of 512 matrix-pipe
// cycles:
//   phase 1  fp16 main term : 2 k-steps x 8 v_mfma_f32_32x32x16_f16          | meanwhile: the Q fragments of this K-tile
//            s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier    <- K-tile t+1 landed; every read of this stage is done
//   phase 2  fp8 cross terms: 8 v_mfma_scale_f32_32x32x64_f8f6f4              | meanwhile: DMA of K-tile t+2 into THIS
//                                                                               stage, H fragments of K-tile t+1
// 96 fragment VGPRs + 128 accumulators, the barrier between phases whose operands are in registers, as in bf16x3.
#include <stdlib.h>

#include "alvq_common.h"
#include "conv_tile.h"
#include "f16mx_common.h"
#include "nlc_host.h"

namespace alvq {

struct ConvFxArgs {
  ConvBArgs b;                        // H planes (and everything shared); mask_bits / bits_out unused
  long x_plane, wp_plane, y_plane;    // element (u16) offsets from an H plane to its Q plane
  int ea, eb;                         // E8M0 scale exponents: weights (A operand), activations / gradients (B operand and outputs)
  const float* out_scale;             // OUT == 1: device scalar multiplied into the fp32 output (undoes a loss scale), or null
  int* range_flag;                    // sticky device flag, |= 4 when a stored H reached fp16's limit
  unsigned long long* stamps;         // DBG instantiations, ALVQ_FX_DBG & 256: per workgroup {start, staged, main loop done, end} (100 MHz)
  int dbg;                            // switches of the DBG instantiations (ALVQ_FX_DBG), timing experiments only: 1 no in-loop
                                      // DMA, 2 no in-loop fragment reads, 4 no wait + barrier, 8 no epilogue, 16 / 32 no fp16 /
                                      // no fp8 MFMAs, 256 phase stamps (results intact), 512 stamps + the epilogue's stores removed
};

// 16 consecutive channels of one row, reconstructed from an f16mx tensor: += H + lo8 * S_lo.  ph -> the row's H at the
// first channel, pq -> the 64-byte Q chunk position of that channel (hi8; lo8 at +32).
__device__ __forceinline__ void fx_join16(const u32x4& h0, const u32x4& h1, const u32x4& ql, float s_lo, float (&v)[16]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a0, a1, b0, b1;
    fx_join2(h0[e], ql[e >> 1], (e & 1) * 2, s_lo, a0, a1);
    fx_join2(h1[e], ql[2 + (e >> 1)], (e & 1) * 2, s_lo, b0, b1);
    v[2 * e] += a0;
    v[2 * e + 1] += a1;
    v[8 + 2 * e] += b0;
    v[8 + 2 * e + 1] += b1;
  }
}
__device__ __forceinline__ void fx_load_add16(const u16* ph, const unsigned char* pq, float s_lo, float (&v)[16]) {
  const u32x4 h0 = *(const u32x4*)ph, h1 = *(const u32x4*)(ph + 8);
  const u32x4 ql = *(const u32x4*)(pq + 32);
  fx_join16(h0, h1, ql, s_lo, v);
}

// Store 16 consecutive channels of one row (H: 32 bytes, hi8 / lo8: 16 bytes each) and return the packed H words (the
// sign bits of a ReLU'd output are derived from them, fx_sign_bits_of_h).
__device__ __forceinline__ void fx_put16(u16* ph, unsigned char* pq, const unsigned (&h)[8], const unsigned (&qh)[4],
                                         const unsigned (&ql)[4]) {
  *(u32x4*)ph = u32x4{h[0], h[1], h[2], h[3]};
  *(u32x4*)(ph + 8) = u32x4{h[4], h[5], h[6], h[7]};
  *(u32x4*)pq = u32x4{qh[0], qh[1], qh[2], qh[3]};
  *(u32x4*)(pq + 32) = u32x4{ql[0], ql[1], ql[2], ql[3]};
}
template <bool NOSTORE = false>
__device__ __forceinline__ void fx_store16(u16* ph, unsigned char* pq, float s_hi, float s_lo, const float (&v)[16], unsigned (&h)[8]) {
  unsigned qh[4], ql[4];
  fx_split<16>(v, s_hi, s_lo, h, qh, ql);
  if (NOSTORE) {   // timing ablation (ALVQ_FX_DBG & 512): the conversions stay, the stores go
#pragma unroll
    for (int e = 0; e < 4; ++e) asm volatile("" ::"v"(h[e]), "v"(h[4 + e]), "v"(qh[e]), "v"(ql[e]));
    return;
  }
  fx_put16(ph, pq, h, qh, ql);
}

// A 32 x 32 accumulator fragment (lane (j, h): row j, channels (q & 3) + 8 (q >> 2) + 4 h) -> 16 consecutive channels
// 16 h .. 16 h + 15 of row j, by one lane swap per register pair.
__device__ __forceinline__ void fx_frag_to_row16(const f32x16& c, float (&v)[16]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const u32x2 ra = __builtin_amdgcn_permlane32_swap(__float_as_uint(c[e]), __float_as_uint(c[8 + e]), false, false);
    const u32x2 rb = __builtin_amdgcn_permlane32_swap(__float_as_uint(c[4 + e]), __float_as_uint(c[12 + e]), false, false);
    v[e] = __uint_as_float(ra[0]);
    v[4 + e] = __uint_as_float(ra[1]);
    v[8 + e] = __uint_as_float(rb[0]);
    v[12 + e] = __uint_as_float(rb[1]);
  }
}
// one v_max_f32 per value (fmaxf costs a second one: the compiler canonicalises its operand first)
__device__ __forceinline__ void fx_relu16(float (&v)[16]) {
#pragma unroll
  for (int e = 0; e < 16; ++e) asm("v_max_f32 %0, 0, %1" : "=v"(v[e]) : "v"(v[e]));
}

// Operand loads come FIRST and in bulk: one load -> use -> store chain per 32-channel tile made the epilogue a string of
// eight L2 / HBM round trips (17 us per workgroup on an otherwise idle chip, before any bandwidth limit).  The skip and
// mask operands of a whole 32-row block (four tiles, 48 + 32 registers -- the fragment registers are free by now) are
// requested at once, and the second row block's while the first is being converted and stored.  Rows outside the data
// (gap / tail rows: every plane holds them, as zeros) are loaded like any other and zeroed by a select, so the code has
// no divergent branch.
struct FxEpiLoads {
  u32x4 h0[4], h1[4], ql[4];   // skip1: H (2 x 16 B) and lo8 of 16 channels, per 32-channel tile
  u32x4 m0[4], m1[4];          // mask as a tensor: H
  unsigned mb[4];              // mask as bits
};

template <int NIN, int DBG = 0>
__device__ __forceinline__ void wave_epilogue_fx(const ConvFxArgs& ax, const f32x16 (&acc)[4][2], int m0, int r0, int lane, int wm0,
                                                 int wn0) {
  const ConvBArgs& a = ax.b;
  const int j = lane & 31, h = lane >> 5;
  const int Lp1 = a.L + 1, ndata = a.B * Lp1;
  const float s_lo = fx_pow2(ax.eb - FX_LO_SHIFT), s_hi = fx_pow2(ax.eb);
  fx_saturating_conversions();
  const int cb0 = m0 + wm0 + 16 * h;
  // Everything below addresses a row block through pointers to (row, channel cb0) computed once; a tile adds the
  // constants 32 mi channels = 64 mi bytes of H, one Q chunk (64 bytes) per tile, 4 mi bytes of sign bits.
  const long qo0 = fx_q_off(cb0);
  FxEpiLoads ld[NIN];
  unsigned watch = 0;
  // per row block, once (the row -> (b, l) division is ~20 VALU instructions): is this lane's row a data row; does the
  // block hold any row that is not
  bool okr[NIN], gapsr[NIN];
#pragma unroll
  for (int ni = 0; ni < NIN; ++ni) {
    int b, l;
    okr[ni] = row_valid(r0 + wn0 + ni * 32 + j, Lp1, ndata, &b, &l);
    gapsr[ni] = !__all(okr[ni]);
  }
  auto request = [&](int ni) {
    const long ro = (long)(r0 + wn0 + ni * 32 + j) * a.Mop;
    const u16* s1h = a.skip1 + ro + cb0;
    const unsigned char* s1q = (const unsigned char*)(a.skip1 + ax.y_plane) + ro * 2 + qo0 + 32;
    const u16* mkh = a.mask + ro + cb0;
    const unsigned char* mkb = a.mask_bits + ((ro + cb0) >> 3);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      if (m0 + wm0 + mi * 32 >= a.Mop) continue;        // Mop % 64 == 0: a 32-channel tile is inside or outside as a whole
      if (a.skip1) {
        ld[ni].h0[mi] = *(const u32x4*)(s1h + mi * 32);
        ld[ni].h1[mi] = *(const u32x4*)(s1h + mi * 32 + 8);
        ld[ni].ql[mi] = *(const u32x4*)(s1q + mi * 64);
      }
      if (a.mask_bits) {   // one bit per element, left behind by the ReLU'd launch that made the tensor: 1/16 of its H plane
        ld[ni].mb[mi] = *(const unsigned short*)(mkb + mi * 4);
      } else if (a.mask) {
        ld[ni].m0[mi] = *(const u32x4*)(mkh + mi * 32);
        ld[ni].m1[mi] = *(const u32x4*)(mkh + mi * 32 + 8);
      }
    }
  };
  auto tile = [&](int ni, int mi) {
    if (m0 + wm0 + mi * 32 >= a.Mop) return;
    const bool ok = okr[ni], gaps = gapsr[ni];
    const long ro = (long)(r0 + wn0 + ni * 32 + j) * a.Mop;
    const long hoff = ro + cb0 + mi * 32;                 // elements from a plane's start to this lane's 16 channels
    const long qoff = ro * 2 + qo0 + mi * 64;             // bytes into the Q plane
    float v[16];
    fx_frag_to_row16(acc[mi][ni], v);
    if (a.bias) {
      const int cb = cb0 + mi * 32;
      if (m0 + wm0 + mi * 32 + 32 <= a.M) {              // the whole 32-channel tile is real channels: four 16-byte loads
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 bq = *(const f32x4*)(a.bias + cb + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * q + e] += bq[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] += (cb + e < a.M) ? a.bias[cb + e] : 0.f;
      }
    }
    if (a.skip1) fx_join16(ld[ni].h0[mi], ld[ni].h1[mi], ld[ni].ql[mi], s_lo, v);
    if (a.skip2) fx_load_add16(a.skip2 + hoff, (const unsigned char*)(a.skip2 + ax.y_plane) + qoff, s_lo, v);
    if (a.relu & 1) fx_relu16(v);
    if (a.mask_bits) {     // sign-extend bit e to a word (v_bfe_i32) and AND: two VALU instructions per element; written
                           // as asm because the compiler turns the C form into and + compare + select with wait states
      const unsigned bt = ld[ni].mb[mi];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        unsigned m;
        asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(bt), "n"(e));
        v[e] = __uint_as_float(__float_as_uint(v[e]) & m);
      }
    } else if (a.mask) {   // the sign of a split value is the sign of its H plane (fp16 reaches 6e-8; smaller activations are zero)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[2 * e] = fx_h2f_lo(ld[ni].m0[mi][e]) > 0.f ? v[2 * e] : 0.f;
        v[2 * e + 1] = fx_h2f_hi(ld[ni].m0[mi][e]) > 0.f ? v[2 * e + 1] : 0.f;
        v[8 + 2 * e] = fx_h2f_lo(ld[ni].m1[mi][e]) > 0.f ? v[8 + 2 * e] : 0.f;
        v[8 + 2 * e + 1] = fx_h2f_hi(ld[ni].m1[mi][e]) > 0.f ? v[8 + 2 * e + 1] : 0.f;
      }
    }
    if (gaps) {                            // one 32-row block in sixteen holds a gap row: gap / tail rows stay zero
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = ok ? v[e] : 0.f;
    }
    unsigned hw[8];
    if (DBG && (ax.dbg & 512)) fx_store16<true>(a.y + hoff, (unsigned char*)(a.y + ax.y_plane) + qoff, s_hi, s_lo, v, hw);
    else fx_store16(a.y + hoff, (unsigned char*)(a.y + ax.y_plane) + qoff, s_hi, s_lo, v, hw);
#pragma unroll
    for (int e = 0; e < 8; ++e) fp16_watch(watch, hw[e]);
    if (a.bits_out) *(unsigned short*)(a.bits_out + (hoff >> 3)) = (unsigned short)fx_sign_bits_of_h(hw);
    if (a.y2) {
      fx_load_add16(a.post + hoff, (const unsigned char*)(a.post + ax.y_plane) + qoff, s_lo, v);
      if (gaps) {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = ok ? v[e] : 0.f;
      }
      fx_store16(a.y2 + hoff, (unsigned char*)(a.y2 + ax.y_plane) + qoff, s_hi, s_lo, v, hw);
    }
  };
  request(0);
  __builtin_amdgcn_sched_barrier(0);
  tile(0, 0);
  tile(0, 1);
  if (NIN > 1) {       // two tiles' accumulators and loads have been retired: room for the second row block's requests
    __builtin_amdgcn_sched_barrier(0);
    request(NIN - 1);
    __builtin_amdgcn_sched_barrier(0);
  }
  tile(0, 2);
  tile(0, 3);
  if (NIN > 1) {
    tile(NIN - 1, 0);
    tile(NIN - 1, 1);
    tile(NIN - 1, 2);
    tile(NIN - 1, 3);
  }
  fp16_report(watch, ax.range_flag);
}

// wave_epilogue_fx for the operand sets the forward launches of a train step are made of, on an m-tile that lies inside
// Mop: EPI == 1 no operand, 2 bias alone, 3 skip1 alone (ReLU and the sign bits of the output either way, at run time: they
// load nothing).  The other operands do not exist here -- no register is held for them and no branch tests them.  Same values
// combined in the same order and stored to the same addresses as the general body; what differs is that no load is
// issued behind one of the wave's own stores (conv1d_bf16x3.hip, wave_epilogue_x3_ordered, says why that matters):
//  * the bias is added into the accumulators in front of everything.  Lane (j, h) of fragment mi holds channels
//    (q & 3) + 8 (q >> 2) + 4 h of both row blocks, so a fragment's bias is four 16-byte loads, and acc + bias is the same
//    float on either side of the lane swap.  The tiles then load nothing.
//  * skip1 goes one row block ahead through ONE 48-register buffer: the second block is requested after the first has
//    been converted (64 registers of H / hi8 / lo8 words, while its 64 accumulators die) and before it is stored.
template <int NIN, int EPI>
__device__ __forceinline__ void wave_epilogue_fx_set(const ConvFxArgs& ax, f32x16 (&acc)[4][2], int m0, int r0, int lane, int wm0,
                                                     int wn0) {
  static_assert(EPI >= 1 && EPI <= 3, "1 no operand, 2 bias, 3 skip1");
  const ConvBArgs& a = ax.b;
  const int j = lane & 31, h = lane >> 5;
  const int Lp1 = a.L + 1, ndata = a.B * Lp1;
  const float s_lo = fx_pow2(ax.eb - FX_LO_SHIFT), s_hi = fx_pow2(ax.eb);
  fx_saturating_conversions();
  const int cb0 = m0 + wm0 + 16 * h;
  const long qo0 = fx_q_off(cb0);
  unsigned watch = 0;
  bool okr[NIN], gapsr[NIN];
#pragma unroll
  for (int ni = 0; ni < NIN; ++ni) {
    int b, l;
    okr[ni] = row_valid(r0 + wn0 + ni * 32 + j, Lp1, ndata, &b, &l);
    gapsr[ni] = !__all(okr[ni]);
  }
  u32x4 s1h0[4], s1h1[4], s1ql[4];   // skip1: H (2 x 16 B) and lo8 of 16 channels, per 32-channel tile
  auto request = [&](int ni) {
    const long ro = (long)(r0 + wn0 + ni * 32 + j) * a.Mop;
    const u16* s1h = a.skip1 + ro + cb0;
    const unsigned char* s1q = (const unsigned char*)(a.skip1 + ax.y_plane) + ro * 2 + qo0 + 32;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      s1h0[mi] = *(const u32x4*)(s1h + mi * 32);
      s1h1[mi] = *(const u32x4*)(s1h + mi * 32 + 8);
      s1ql[mi] = *(const u32x4*)(s1q + mi * 64);
    }
  };
  // one tile up to its stored words; skip1 of row block ni is in the buffer
  auto convert = [&](int ni, int mi, unsigned (&hw)[8], unsigned (&qh)[4], unsigned (&ql)[4]) {
    float v[16];
    fx_frag_to_row16(acc[mi][ni], v);
    if (EPI == 3) fx_join16(s1h0[mi], s1h1[mi], s1ql[mi], s_lo, v);
    if (a.relu & 1) fx_relu16(v);
    if (gapsr[ni]) {                       // one 32-row block in sixteen holds a gap row: gap / tail rows stay zero
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = okr[ni] ? v[e] : 0.f;
    }
    fx_split<16>(v, s_hi, s_lo, hw, qh, ql);
#pragma unroll
    for (int e = 0; e < 8; ++e) fp16_watch(watch, hw[e]);
  };
  auto store = [&](int ni, int mi, const unsigned (&hw)[8], const unsigned (&qh)[4], const unsigned (&ql)[4]) {
    const long ro = (long)(r0 + wn0 + ni * 32 + j) * a.Mop;
    const long hoff = ro + cb0 + mi * 32;                 // elements from a plane's start to this lane's 16 channels
    const long qoff = ro * 2 + qo0 + mi * 64;             // bytes into the Q plane
    fx_put16(a.y + hoff, (unsigned char*)(a.y + ax.y_plane) + qoff, hw, qh, ql);
    if (a.bits_out) *(unsigned short*)(a.bits_out + (hoff >> 3)) = (unsigned short)fx_sign_bits_of_h(hw);
  };
  auto tile = [&](int ni, int mi) {
    unsigned hw[8], qh[4], ql[4];
    convert(ni, mi, hw, qh, ql);
    store(ni, mi, hw, qh, ql);
  };

  if (EPI == 3) request(0);
  if (EPI == 2) {
    f32x4 bq[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int c0 = m0 + wm0 + mi * 32;
      if (c0 + 32 <= a.M) {                               // the whole 32-channel tile is real channels
#pragma unroll
        for (int k = 0; k < 4; ++k) bq[mi][k] = *(const f32x4*)(a.bias + c0 + 8 * k + 4 * h);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e) bq[mi][k][e] = (c0 + 8 * k + 4 * h + e < a.M) ? a.bias[c0 + 8 * k + 4 * h + e] : 0.f;
      }
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < NIN; ++ni)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[mi][ni][q] += bq[mi][q >> 2][q & 3];
  }
  __builtin_amdgcn_sched_barrier(0);
  if (EPI == 3 && NIN > 1) {
    unsigned hw[4][8], qh[4][4], ql[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) convert(0, mi, hw[mi], qh[mi], ql[mi]);
    __builtin_amdgcn_sched_barrier(0);
    request(NIN - 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) store(0, mi, hw[mi], qh[mi], ql[mi]);
  } else {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) tile(0, mi);
  }
  if (NIN > 1) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) tile(NIN - 1, mi);
  }
  fp16_report(watch, ax.range_flag);
}

// DBG: 1 run-time ablation switches, 2 also no fp16 MFMAs, 3 also no fp8 MFMAs (timing experiments, tools/ablate_f16mx.sh).
// NIN: 32-row blocks per wave.  2 = the 256-row tile; 1 = a 128-row tile (a wave owns 128 x 32) for launches whose 256-row
// grid would leave CUs idle (one m-tile: M <= 256, or few rows) -- twice the workgroups at 5/4 instead of 6/8 fragment
// reads per MFMA.
// MIN: 32-channel blocks per wave.  4 = the 256-channel m-tile; 2 = a 128-channel m-tile (a wave owns 64 x 32, with
// NIN = 1) for layers of at most 128 output channels, whose 256-wide tile would spend half of its MFMAs on padding.
// EPI: operand set of the f16mx output's epilogue.  0 = any (wave_epilogue_fx tests every operand at run time); 1 / 2 / 3 =
// none / bias alone / skip1 alone (wave_epilogue_fx_set).  A parameter of the KERNEL: with the general body in the same
// kernel the register allocator sized the whole kernel for it (255 VGPRs and 288 bytes of scratch against 68).
template <int OUT, int KW, int DBG = 0, int NIN = 2, int MIN = 4, int EPI = 0>
__global__ __launch_bounds__(512, 2) void conv1d_f16mx_kernel(ConvFxArgs ax) {
  typedef ConvRings G;
  constexpr int RT = 128 * NIN;          // rows per workgroup
  constexpr int MT = 64 * MIN;           // output channels per workgroup
  const int dbg = DBG ? ax.dbg : 0;
  const ConvBArgs& a = ax.b;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave >> 2) * 32 * MIN, wn0 = (wave & 3) * 32 * NIN;

  const ConvTileOrigin o = conv_tile_origin<MT, RT>(a);
  const int m0 = o.m0, r0 = o.r0;
  const int Cp = a.Cp;
  // ---- DMA sources (ConvRingStager, conv_tile.h, says what each is): plane 0 = H, plane 1 = Q; the pieces are issued one at a
  // time so that each can sit in the shadow of an MFMA
  const int srow = slab64_lane(lane).row;
  const unsigned lane_off = slab64_lane_off(lane, Cp);
  const long tap_w = (long)a.Mp128 * Cp * 2;
  const long row16 = (long)Cp * 32;
  const long wpl = ax.wp_plane * 2, xpl = ax.x_plane * 2;
  const char* const wb = (const char*)(a.wp + ((long)m0 + wave * 32) * Cp);
  const char* const xb = (const char*)(a.x + ((long)r0 - (KW - 1) / 2 + wave * 32) * Cp);
  const ConvRingStager<KW, MT, RT, true> st(wave, srow, lane_off, tap_w, row16, wpl, xpl, wb, xb);

  // ---- fragment reads for the 32x32 shapes: lane (r = lane & 31, g = lane >> 5) takes the 16-byte groups g and 2 + g of
  // row r of a 32-row block.  H slab: group g = k-step 0 (channels 8g..8g+7), group 2+g = k-step 1.  Q slab: group g =
  // hi8[16g..16g+15], group 2+g = lo8[16g..16g+15]; the A operand wants (hi8, lo8), the B operand (lo8, hi8), so that
  // block 0 of the scaled MFMA pairs A.hi8 with B.lo8 and block 1 A.lo8 with B.hi8.  The slot swizzle of the staging makes
  // the un-shifted reads conflict-free for this lane pattern too; the activation reads of tap t use slab row r + t.
  const int r32 = lane & 31, g = lane >> 5;
  int offA[2], offB[KW][2];
  offA[0] = slab64_frag32(r32, g, 0);
  offA[1] = slab64_frag32(r32, 2 + g, 0);
#pragma unroll
  for (int t = 0; t < KW; ++t) {
    offB[t][0] = slab64_frag32(r32, g, t);
    offB[t][1] = slab64_frag32(r32, 2 + g, t);
  }
  const unsigned char* const abase = lds + wm0 * 64;
  const unsigned char* const bbase = lds + G::XBASE + wn0 * 64;
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  f16x8_t aH[4][2], bH[2][2];
  i32x8 aQ[4], bQ[2];
#define FX_RDH_A(WS, MI, KS) if ((MI) < MIN) aH[MI][KS] = *(const f16x8_t*)(abase + (WS) * G::WSTAGE + (MI) * 2048 + offA[KS]);
#define FX_RDH_B(XS, TAP, NI, KS) if ((NI) < NIN) bH[NI][KS] = *(const f16x8_t*)(bbase + (XS) * G::XSTAGE + (NI) * 2048 + offB[TAP][KS]);
#define FX_RDQ(DST, P, FIRST, SECOND)                                                           \
  {                                                                                             \
    const i32x4 q0_ = *(const i32x4*)((P) + (FIRST)), q1_ = *(const i32x4*)((P) + (SECOND));    \
    DST = __builtin_shufflevector(q0_, q1_, 0, 1, 2, 3, 4, 5, 6, 7);                            \
  }
#define FX_RDQ_A(WS, MI) if ((MI) < MIN) FX_RDQ(aQ[MI], abase + (WS) * G::WSTAGE + G::SLAB + (MI) * 2048, offA[0], offA[1])
#define FX_RDQ_B(XS, TAP, NI) if ((NI) < NIN) FX_RDQ(bQ[NI], bbase + (XS) * G::XSTAGE + G::XSLAB + (NI) * 2048, offB[TAP][1], offB[TAP][0])

  // block scales of the fp8 MFMA: lanes 0-31 supply block 0, lanes 32-63 block 1.  Opaque to the compiler so that it keeps
  // them in registers instead of re-materialising them by VALU moves in front of the inline-asm MFMAs (no hazard padding
  // happens for instructions it cannot see).
  int sa = g ? ax.ea - FX_LO_SHIFT : ax.ea, sb = g ? ax.eb : ax.eb - FX_LO_SHIFT;
  asm volatile("" : "+v"(sa), "+v"(sb));

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][jn][q] = 0.f;
#define FX_H(MI, NI, KS) if (DBG != 2 && (NI) < NIN && (MI) < MIN) asm("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc[MI][NI]) : "v"(aH[MI][KS]), "v"(bH[NI][KS]));
#define FX_Q(MI, NI)                                                                          \
  if ((NI) < NIN && (MI) < MIN && DBG != 3)                                                                        \
    asm("v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"            \
        : "+v"(acc[MI][NI]) : "v"(aQ[MI]), "v"(bQ[NI]), "v"(sa), "v"(sb));
#define FX_SB __builtin_amdgcn_sched_barrier(0);

  const int nch = Cp / G::K;        // chunks; even (Cp % 64 == 0)
  const int n = nch * KW;           // K-tiles
  const bool early = wave < 4;      // the two waves of a SIMD issue their DMA at different points of phase 2

  unsigned long long st0 = 0, st1 = 0, st2 = 0;
  if (DBG) st0 = __builtin_amdgcn_s_memrealtime();
  // ---- prologue: chunk 0's activation slabs, K-tiles 0 and 1 (and, for width 1, chunk 1's slabs) staged; H fragments of
  // K-tile 0 in registers
  st.prologue(lds, n, nch);
  if (DBG) st1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
  for (int mi = 0; mi < MIN; ++mi) { FX_RDH_A(0, mi, 0) FX_RDH_A(0, mi, 1) }
#pragma unroll
  for (int ni = 0; ni < NIN; ++ni) { FX_RDH_B(0, 0, ni, 0) FX_RDH_B(0, 0, ni, 1) }

  // One K-tile: weights in stage WS, activations in stage XS read at tap TAP; the next K-tile's are (NWS, NXS, NTAP).
  // TW = the K-tile whose weights are staged behind this tile's barrier (into the weight stage this tile occupied), or
  // -1; XC / XP = chunk and plane of the activation slab staged here, or XC = -1.
  // Every LDS read and every DMA piece sits in the shadow of ONE MFMA (at most two 16-byte reads or one DMA piece plus
  // two reads per gap): issued in bursts -- all twelve reads of a phase in a row, by both waves of a SIMD at the same
  // point of the program -- they left the matrix pipe idle for the length of the burst (measured: 17 % of the kernel).
  // Reads are ordered by first use; the early / late halves of the workgroup place their DMA pieces in different gaps.
#define FX_RD(X_) if (!(dbg & 2)) { X_ }
#define FX_DMA_E(X_) if (early && !(dbg & 1)) { X_ }
#define FX_DMA_L(X_) if (!early && !(dbg & 1)) { X_ }
#define FX_TILE(WS, XS, TAP, NWS, NXS, NTAP, TW, XC, XP)                                                                 \
  FX_H(0, 0, 0) FX_SB FX_RD(FX_RDQ_B(XS, TAP, 0)) FX_SB                                                                   \
  FX_H(0, 1, 0) FX_SB FX_RD(FX_RDQ_A(WS, 0)) FX_SB                                                                        \
  FX_H(1, 0, 0) FX_SB FX_RD(FX_RDQ_B(XS, TAP, 1)) FX_SB                                                                   \
  FX_H(1, 1, 0) FX_SB FX_RD(FX_RDQ_A(WS, 1)) FX_SB                                                                        \
  FX_H(2, 0, 0) FX_SB FX_RD(FX_RDQ_A(WS, 2)) FX_SB                                                                        \
  FX_H(2, 1, 0) FX_SB FX_RD(FX_RDQ_A(WS, 3)) FX_SB                                                                        \
  FX_H(3, 0, 0) FX_H(3, 1, 0)                                                                                            \
  FX_H(0, 0, 1) FX_H(0, 1, 1) FX_H(1, 0, 1) FX_H(1, 1, 1) FX_H(2, 0, 1) FX_H(2, 1, 1) FX_H(3, 0, 1) FX_H(3, 1, 1) FX_SB   \
  if (!(dbg & 4)) {                                                                                                      \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                          \
    __builtin_amdgcn_s_barrier();                                                                                        \
  }                                                                                                                      \
  FX_Q(0, 0) FX_SB FX_DMA_E(if ((TW) >= 0) st.pieceW(lds, TW, 0);) FX_RD(FX_RDH_B(NXS, NTAP, 0, 0) FX_RDH_A(NWS, 0, 0)) FX_SB     \
  FX_Q(0, 1) FX_SB FX_DMA_E(if ((TW) >= 0) st.pieceW(lds, TW, 1);) FX_RD(FX_RDH_B(NXS, NTAP, 1, 0) FX_RDH_A(NWS, 1, 0)) FX_SB     \
  FX_Q(1, 0) FX_SB FX_DMA_E(if ((TW) >= 0) st.pieceW(lds, TW, 2);) FX_RD(FX_RDH_A(NWS, 2, 0) FX_RDH_A(NWS, 3, 0)) FX_SB           \
  FX_Q(1, 1) FX_SB FX_DMA_E(if ((TW) >= 0) st.pieceW(lds, TW, 3);) FX_RD(FX_RDH_B(NXS, NTAP, 0, 1) FX_RDH_B(NXS, NTAP, 1, 1)) FX_SB \
  FX_Q(2, 0) FX_SB FX_DMA_L(if ((TW) >= 0) { st.pieceW(lds, TW, 0); st.pieceW(lds, TW, 1); }) FX_RD(FX_RDH_A(NWS, 0, 1) FX_RDH_A(NWS, 1, 1)) FX_SB \
  FX_Q(2, 1) FX_SB FX_DMA_L(if ((TW) >= 0) { st.pieceW(lds, TW, 2); st.pieceW(lds, TW, 3); }) FX_RD(FX_RDH_A(NWS, 2, 1) FX_RDH_A(NWS, 3, 1)) FX_SB \
  FX_Q(3, 0) FX_SB if (!(dbg & 1) && (XC) >= 0) { st.pieceX(lds, XC, XP, 0); st.pieceX(lds, XC, XP, 1); st.pieceX(lds, XC, XP, 2); } FX_SB       \
  FX_Q(3, 1) FX_SB if (KW == 1 && !(dbg & 1) && (XC) >= 0) { st.pieceX(lds, XC, 1, 0); st.pieceX(lds, XC, 1, 1); } FX_SB

  if (KW == 3) {
    // two chunks (six K-tiles) per iteration so that every stage index is a constant.  The next chunk's activation slabs
    // are staged behind the barriers of this chunk's taps 0 (H plane) and 1 (Q plane): its stage was released by the
    // previous chunk's last barrier, and it is first read behind this chunk's last one.
    for (int c = 0; c < nch; c += 2) {
      const int t = 3 * c;
      const int x1 = c + 1 < nch ? c + 1 : -1, x2 = c + 2 < nch ? c + 2 : -1;
      FX_TILE(0, 0, 0, 1, 0, 1, (t + 2 < n ? t + 2 : -1), x1, 0)
      FX_TILE(1, 0, 1, 0, 0, 2, (t + 3 < n ? t + 3 : -1), x1, 1)
      FX_TILE(0, 0, 2, 1, 1, 0, (t + 4 < n ? t + 4 : -1), -1, 0)
      FX_TILE(1, 1, 0, 0, 1, 1, (t + 5 < n ? t + 5 : -1), x2, 0)
      FX_TILE(0, 1, 1, 1, 1, 2, (t + 6 < n ? t + 6 : -1), x2, 1)
      FX_TILE(1, 1, 2, 0, 0, 0, (t + 7 < n ? t + 7 : -1), -1, 0)
    }
  } else {
    // width 1: a chunk is one K-tile; both planes of chunk t + 2 follow its weights (last two gaps of the tile)
    for (int t = 0; t < n; t += 2) {
      const int a2 = t + 2 < n ? t + 2 : -1, a3 = t + 3 < n ? t + 3 : -1;
      FX_TILE(0, 0, 0, 1, 1, 0, a2, a2, 0)
      FX_TILE(1, 1, 0, 0, 0, 0, a3, a3, 0)
    }
  }
#undef FX_TILE
#undef FX_DMA_L
#undef FX_DMA_E
#undef FX_RD
#undef FX_SB
#undef FX_Q
#undef FX_H
#undef FX_RDQ_B
#undef FX_RDQ_A
#undef FX_RDQ
#undef FX_RDH_B
#undef FX_RDH_A
  // the compiler's hazard recogniser does not see inside the asm MFMAs: cover the MFMA-result -> VALU-read wait states
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");

  if (DBG) st2 = __builtin_amdgcn_s_memrealtime();
  if (dbg & 8) {
    if (acc[0][0][0] == 12345.678f) a.y[0] = 1;   // keep the accumulators alive
    return;
  }
  if (OUT == 0) {
    if constexpr (EPI != 0) wave_epilogue_fx_set<NIN, EPI>(ax, acc, m0, r0, lane, wm0, wn0);
    else wave_epilogue_fx<NIN, DBG>(ax, acc, m0, r0, lane, wm0, wn0);
    if (DBG && (dbg & (256 | 512))) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the stores have left
      __syncthreads();
      if (tid == 0) {
        unsigned long long* o = ax.stamps + (long)blockIdx.x * 4;
        o[0] = st0; o[1] = st1; o[2] = st2; o[3] = __builtin_amdgcn_s_memrealtime();
      }
    }
    return;
  }
  __syncthreads();   // the C slab overlays the stages: the trailing fragment reads of every wave must be done
  // ---- OUT == 1 (optional output scale): 64-row slabs; a 32 x 32 fragment is four 16-byte groups of consecutive m per lane
  conv_store_ncl<true, MT, RT>(a, lds, m0, r0, tid, ax.out_scale, [&](float* Cs, int slab) {
    if ((wn0 >> 6) != slab) return;
#pragma unroll
    for (int mi = 0; mi < MIN; ++mi)
#pragma unroll
      for (int ni = 0; ni < NIN; ++ni)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int rl = (wn0 & 63) + ni * 32 + r32, ml = wm0 + mi * 32 + 8 * q4 + 4 * g;
          *(f32x4*)(Cs + rl * C_SLAB_STRIDE + ml) =
              f32x4{acc[mi][ni][4 * q4], acc[mi][ni][4 * q4 + 1], acc[mi][ni][4 * q4 + 2], acc[mi][ni][4 * q4 + 3]};
        }
  });
}

// ------------------------------------------------------------------------------------------------ boundary conversions
// Sticky range flag of the format (one int per device, in the code object's own data segment -- not an allocation):
// bit 0 = a value of magnitude >= 65504 (fp16's largest finite value; it was stored saturated), bit 1 = a NaN, seen by a
// conversion INTO the format (model inputs, gradients entering a backward chain); bit 2 = a value PRODUCED inside a chain
// (an activation, or a loss-scaled gradient that outgrew the 2^8 headroom) reached the limit or is a NaN -- watched by
// the epilogues of the f16mx and fp16 convolutions.  Read / cleared by alvq_f16mx_range_flag.
// Round 4: the flag has two words.  g_fx_range_flag collects the bits raised since the last GUARDED optimiser advance
// (alvq_adam_advance_f32 with a skip slot: the start of a Trainer step), so that a step's last launch can turn "did THIS
// step saturate" into the skip slot of the flat gradient buffer (alvq_range_flag_to_slot); the advance folds the bits into
// g_fx_range_sticky.  alvq_f16mx_range_flag reports / clears the union.
__device__ int g_fx_range_flag = 0;
__device__ int g_fx_range_sticky = 0;

int* fx_range_flag_ptr() {
  static int* cache[64] = {};
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) d = 0;
  if (!cache[d]) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_fx_range_flag)) == hipSuccess) cache[d] = (int*)p;
  }
  return cache[d];
}

int* fx_range_sticky_ptr() {
  static int* cache[64] = {};
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) d = 0;
  if (!cache[d]) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_fx_range_sticky)) == hipSuccess) cache[d] = (int*)p;
  }
  return cache[d];
}

__global__ void fx_range_flag_kernel(int* out, int reset) {
  *out = g_fx_range_flag | g_fx_range_sticky;
  if (reset) { g_fx_range_flag = 0; g_fx_range_sticky = 0; }
}

// (B,C,L) fp32 -> f16mx NLC planes, optionally multiplied by a device scalar (the loss scale of a backward chain)
__global__ __launch_bounds__(256) void ncl_to_nlc_fx_kernel(const float* x, u16* y, long plane, int B, int C, int L, int Cp,
                                                            int rows_total, int e, const float* scale) {
  __shared__ float tile[32][33];
  fx_saturating_conversions();
  int range = 0;
  const int ct = Cp / 32;
  const int r0 = (blockIdx.x / ct) * 32, c0 = (blockIdx.x % ct) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int Lp1 = L + 1, ndata = B * Lp1;
  const float sc = scale ? *scale : 1.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, row = r0 + tx;
    int b, l;
    const bool ok = row_valid(row, Lp1, ndata, &b, &l) && c < C;
    const float v = ok ? x[((long)b * C + c) * L + l] * sc : 0.f;
    tile[ty + 8 * i][tx] = v;
    range |= (fabsf(v) >= 65504.f ? 1 : 0) | (v != v ? 2 : 0);
  }
  if (__any(range)) {                       // rare: one atomic per wave that saw such a value
    range = wave_or(range);
    if ((threadIdx.x & 63) == 0) atomicOr(&g_fx_range_flag, range);
  }
  __syncthreads();
  // thread (row = tid >> 3, 4 channels at (tid & 7) * 4): 8 bytes of H, 4 of hi8, 4 of lo8
  const int rr = threadIdx.x >> 3, cq = (threadIdx.x & 7) * 4;
  const int row = r0 + rr;
  if (row < rows_total) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = tile[cq + k][rr];
    unsigned h[2], qh[1], ql[1];
    fx_split<4>(v, fx_pow2(e), fx_pow2(e - FX_LO_SHIFT), h, qh, ql);
    *(u32x2*)(y + (long)row * Cp + c0 + cq) = u32x2{h[0], h[1]};
    unsigned char* q = (unsigned char*)(y + plane) + (long)row * Cp * 2 + fx_q_off(c0) + cq;
    *(unsigned*)q = qh[0];
    *(unsigned*)(q + 32) = ql[0];
  }
}

__global__ __launch_bounds__(256) void nlc_to_ncl_fx_kernel(const u16* x, long plane, float* y, int B, int C, int L, int Cp,
                                                            int rows_total, int e, const float* scale) {
  __shared__ float tile[32][33];
  const int ct = Cp / 32;
  const int r0 = (blockIdx.x / ct) * 32, c0 = (blockIdx.x % ct) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int Lp1 = L + 1, ndata = B * Lp1;
  const float sc = scale ? *scale : 1.f, s_lo = fx_pow2(e - FX_LO_SHIFT);
  const int rr = threadIdx.x >> 3, cq = (threadIdx.x & 7) * 4;
  const int rowq = r0 + rr;
  if (rowq < rows_total) {
    const u32x2 h = *(const u32x2*)(x + (long)rowq * Cp + c0 + cq);
    const unsigned ql = *(const unsigned*)((const unsigned char*)(x + plane) + (long)rowq * Cp * 2 + fx_q_off(c0) + cq + 32);
    float v0, v1, v2, v3;
    fx_join2(h[0], ql, 0, s_lo, v0, v1);
    fx_join2(h[1], ql, 2, s_lo, v2, v3);
    tile[rr][cq] = v0 * sc;
    tile[rr][cq + 1] = v1 * sc;
    tile[rr][cq + 2] = v2 * sc;
    tile[rr][cq + 3] = v3 * sc;
  } else {
    tile[rr][cq] = tile[rr][cq + 1] = tile[rr][cq + 2] = tile[rr][cq + 3] = 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, row = r0 + tx;
    int b, l;
    if (row_valid(row, Lp1, ndata, &b, &l) && c < C) y[((long)b * C + c) * L + l] = tile[tx][ty + 8 * i];
  }
}

// out = t > 0 ? dy : 0 on all three parts (16 channels per thread step; the sign of a value is the sign of its H part)
__global__ __launch_bounds__(256) void relu_mask_fx_kernel(const u16* dy, const u16* t, u16* out, long plane, int rows, int Cp) {
  const long n16 = (long)rows * Cp / 16;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) {
    const long row = (i * 16) / Cp;
    const int c = (int)((i * 16) % Cp);
    const long ro = row * Cp;
    const u32x4 m0 = *(const u32x4*)(t + ro + c), m1 = *(const u32x4*)(t + ro + c + 8);
    u32x4 h0 = *(const u32x4*)(dy + ro + c), h1 = *(const u32x4*)(dy + ro + c + 8);
    const unsigned char* qs = (const unsigned char*)(dy + plane) + ro * 2 + fx_q_off(c);
    u32x4 qh = *(const u32x4*)qs, ql = *(const u32x4*)(qs + 32);
    unsigned keep = 0;   // bit k: channel c + k survives
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      keep |= (fx_h2f_lo(m0[e]) > 0.f ? 1u : 0u) << (2 * e) | (fx_h2f_hi(m0[e]) > 0.f ? 1u : 0u) << (2 * e + 1);
      keep |= (fx_h2f_lo(m1[e]) > 0.f ? 1u : 0u) << (8 + 2 * e) | (fx_h2f_hi(m1[e]) > 0.f ? 1u : 0u) << (9 + 2 * e);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned k0 = (keep >> (2 * e)) & 3u, k1 = (keep >> (8 + 2 * e)) & 3u;
      h0[e] &= ((k0 & 1u) ? 0xffffu : 0u) | ((k0 & 2u) ? 0xffff0000u : 0u);
      h1[e] &= ((k1 & 1u) ? 0xffffu : 0u) | ((k1 & 2u) ? 0xffff0000u : 0u);
      const unsigned kb = (keep >> (4 * e)) & 15u;
      const unsigned bm = ((kb & 1u) ? 0xffu : 0u) | ((kb & 2u) ? 0xff00u : 0u) | ((kb & 4u) ? 0xff0000u : 0u) | ((kb & 8u) ? 0xff000000u : 0u);
      qh[e] &= bm;
      ql[e] &= bm;
    }
    *(u32x4*)(out + ro + c) = h0;
    *(u32x4*)(out + ro + c + 8) = h1;
    unsigned char* qd = (unsigned char*)(out + plane) + ro * 2 + fx_q_off(c);
    *(u32x4*)qd = qh;
    *(u32x4*)(qd + 32) = ql;
  }
}

// Loss scale of a backward chain, chosen on the device: state = {S, 1/S, amax bits, -}.  Pass 1 folds |x| into state[2]
// (integer max of the float bits: order-independent, exact); pass 2 turns it into the power of two that puts amax at
// 2^8 -- 2^8 of headroom below fp16's 65504 for growth along the chain, 2^22 above its smallest normal -- and rearms.
__global__ __launch_bounds__(256) void grad_amax_kernel(const float* x, long n, float* state) {
  float m = 0.f;
  const long n4 = n >> 2, stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {      // four independent 16-byte loads in flight per thread
    const f32x4 a = ((const f32x4*)x)[i], b = ((const f32x4*)x)[i + stride], c = ((const f32x4*)x)[i + 2 * stride],
                d = ((const f32x4*)x)[i + 3 * stride];
#pragma unroll
    for (int k = 0; k < 4; ++k) m = fmaxf(fmaxf(m, fmaxf(fabsf(a[k]), fabsf(b[k]))), fmaxf(fabsf(c[k]), fabsf(d[k])));
  }
  for (; i < n4; i += stride) {
    const f32x4 v = ((const f32x4*)x)[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
  }
  for (long j = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; j < n; j += stride) m = fmaxf(m, fabsf(x[j]));
  // one atomic per workgroup (thousands of same-address atomics serialise at the L2: they, not the 26 MB read, set the
  // 51 us this pass took with one atomic per wave on 2048 workgroups)
  __shared__ float wm[4];
  m = block_max<kPairwise4, false>(m, wm);
  if (threadIdx.x == 0) {
    if (m > 0.f) atomicMax((unsigned*)state + 2, __float_as_uint(m));
  }
}
__global__ void grad_scale_kernel(float* state) {
  const unsigned bits = ((unsigned*)state)[2];
  const float amax = __uint_as_float(bits);
  int e = 127;                                        // S = 1 when the gradient is all zero / not finite
  if (amax > 0.f && amax < 3.0e38f) {
    const int ea = (int)((bits >> 23) & 0xff);        // amax in [2^(ea-127), 2^(ea-126))
    e = 127 + 8 - (ea - 127) - 1;                     // S * amax in [2^7, 2^8)
    e = e < 1 ? 1 : (e > 253 ? 253 : e);
  }
  state[0] = fx_pow2(e);
  state[1] = fx_pow2(254 - e);
  ((unsigned*)state)[2] = 0u;
}

}  // namespace alvq

using namespace alvq;

extern "C" int alvq_ncl_to_nlc_f16mx(const float* x, void* y, int B, int C, int L, const float* scale, void* stream) {
  if (int rc = check_nlc_dims("alvq_ncl_to_nlc_f16mx", x && y, B, C, L)) return rc;
  const NlcDims d(B, C, L);
  hipLaunchKernelGGL(ncl_to_nlc_fx_kernel, d.grid32(), dim3(256), 0, (hipStream_t)stream, x, (u16*)y, d.plane, B, C, L, d.Cp, d.rows,
                     FX_E_ACT, scale);
  return check_launch("alvq_ncl_to_nlc_f16mx");
}

extern "C" int alvq_nlc_to_ncl_f16mx(const void* x, float* y, int B, int C, int L, const float* scale, void* stream) {
  if (int rc = check_nlc_dims("alvq_nlc_to_ncl_f16mx", x && y, B, C, L)) return rc;
  const NlcDims d(B, C, L);
  hipLaunchKernelGGL(nlc_to_ncl_fx_kernel, d.grid32(), dim3(256), 0, (hipStream_t)stream, (const u16*)x, d.plane, y, B, C, L, d.Cp,
                     d.rows, FX_E_ACT, scale);
  return check_launch("alvq_nlc_to_ncl_f16mx");
}

extern "C" int alvq_f16mx_range_flag(int* out, int reset, void* stream) {
  ALVQ_REQUIRE(out, ALVQ_EINVAL, "alvq_f16mx_range_flag: null pointer");
  hipLaunchKernelGGL(fx_range_flag_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, out, reset);
  return check_launch("alvq_f16mx_range_flag");
}

extern "C" int alvq_relu_mask_f16mx(const void* dy, const void* t, void* out, int B, int C, int L, void* stream) {
  if (int rc = check_nlc_dims("alvq_relu_mask_f16mx", dy && t && out, B, C, L)) return rc;
  const NlcDims d(B, C, L);
  long gq = ((long)d.rows * d.Cp / 16 + 255) / 256;
  if (gq > 2048) gq = 2048;
  hipLaunchKernelGGL(relu_mask_fx_kernel, dim3((int)gq), dim3(256), 0, (hipStream_t)stream, (const u16*)dy, (const u16*)t, (u16*)out,
                     d.plane, d.rows, d.Cp);
  return check_launch("alvq_relu_mask_f16mx");
}

extern "C" int alvq_grad_scale_f32(const float* x, int64_t n, float* state, void* stream) {
  ALVQ_REQUIRE(x && state, ALVQ_EINVAL, "alvq_grad_scale_f32: null pointer");
  ALVQ_REQUIRE(n > 0, ALVQ_EINVAL, "alvq_grad_scale_f32: n <= 0");
  ALVQ_REQUIRE(((uintptr_t)x & 15) == 0, ALVQ_EINVAL, "alvq_grad_scale_f32: x must be 16-byte aligned");
  long gq = (n / 4 + 256 * 4 - 1) / (256 * 4);
  if (gq > 512) gq = 512;
  if (gq < 1) gq = 1;
  hipLaunchKernelGGL(grad_amax_kernel, dim3((int)gq), dim3(256), 0, (hipStream_t)stream, x, (long)n, state);
  hipLaunchKernelGGL(grad_scale_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
  return check_launch("alvq_grad_scale_f32");
}

// conv1d_f16mx_kernel<OUT, KW, 0, NIN, MIN, EPI> sits at fx_slot(OUT, KW, NIN, MIN, EPI); (NIN, MIN) = (2, 4), (1, 4), (1, 2)
// -- the 256-row tile, the 128-row tile, the 128-row x 128-channel tile -> 0, 1, 2.  The last exists for the fp32-NCL output
// only, and EPI != 0 for the f16mx output only: the fp32-NCL store (conv_store_ncl) is not this file's and has one operand.
static constexpr int fx_slot(int OUT, int KW, int NIN, int MIN, int EPI = 0) {
  return ((((NIN == 1) + (MIN == 2)) * 2 + OUT) * 2 + (KW == 3)) * 4 + EPI;
}
typedef KernelTable<void (*)(ConvFxArgs), 48> FxTable;
static FxTable fx_table() {
  FxTable t;
  for_values<1, 3>([&](auto kw) {
    for_values<0, 1>([&](auto out) { for_values<2, 1>([&](auto nin) {
      t.put(fx_slot(out, kw, nin, 4), conv1d_f16mx_kernel<out, kw, 0, nin, 4>, ConvRings::LDS);
    }); });
    t.put(fx_slot(1, kw, 1, 2), conv1d_f16mx_kernel<1, kw, 0, 1, 2>, ConvRings::LDS);
    for_values<2, 1>([&](auto nin) { for_values<1, 2, 3>([&](auto epi) {
      t.put(fx_slot(0, kw, nin, 4, epi), conv1d_f16mx_kernel<0, kw, 0, nin, 4, epi>, ConvRings::LDS);
    }); });
  });
  return t;
}

extern "C" int alvq_conv1d_f16mx(const void* x, const void* wp, const float* bias, const void* skip1, const void* skip2,
                                 const void* mask, const void* post, void* y, void* y2, float* y_ncl, int B, int C, int M, int L,
                                 int KW, int relu, const void* mask_bits, void* relu_bits_out, const float* out_scale, void* stream) {
  if (int rc = check_conv_args("alvq_conv1d_f16mx", x, wp, skip1, skip2, mask, post, y, y2, y_ncl, B, C, M, L, KW, relu, mask_bits,
                               relu_bits_out, " (and the output scale)"))
    return rc;
  const long rows = alvq_nlc_rows(B, L);
  ConvFxArgs a{{(const u16*)x, (const u16*)wp, bias, (const u16*)skip1, (const u16*)skip2, (const u16*)mask, (const u16*)post,
                (u16*)y, (u16*)y2, y_ncl, B, L, pad_to(C, 64), M, pad_to(M, 64), pad_to(M, WP_ROWS), relu ? 1 : 0,
                (int)(rows / ConvRings::R), pad_to(M, ConvRings::M) / ConvRings::M,   /* rtiles: see below */
                (const unsigned char*)mask_bits, (unsigned char*)relu_bits_out},
               nlc_plane_elems(B, L, C), (long)alvq_packed_weight_elems(M, C, KW), nlc_plane_elems(B, L, M),
               FX_E_W, FX_E_ACT, out_scale, fx_range_flag_ptr(), nullptr, 0};
#ifdef ALVQ_DEBUG_KERNELS   // the ablation / phase-stamp instantiations exist only in the debug library (build.py --debug-kernels)
  static const int dbg_env = getenv("ALVQ_FX_DBG") ? atoi(getenv("ALVQ_FX_DBG")) : 0;   // timing ablations (results are garbage)
#else
  constexpr int dbg_env = 0;
#endif
  a.dbg = dbg_env;
  hipStream_t s = (hipStream_t)stream;
  static const FxTable table = fx_table();
  static DeviceOnce attr;
  if (attr.need()) {
    table.raise_lds_limit();
#ifdef ALVQ_DEBUG_KERNELS
    (void)hipFuncSetAttribute((const void*)conv1d_f16mx_kernel<0, 3, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, ConvRings::LDS);
    (void)hipFuncSetAttribute((const void*)conv1d_f16mx_kernel<0, 1, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, ConvRings::LDS);
    (void)hipFuncSetAttribute((const void*)conv1d_f16mx_kernel<0, 3, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, ConvRings::LDS);
    (void)hipFuncSetAttribute((const void*)conv1d_f16mx_kernel<0, 3, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, ConvRings::LDS);
#endif
  }
  // fewer than ~3/4 of the CUs covered by 256-row tiles (one m-tile: M <= 256; short batches): 128-row tiles
  // (option "fx_rows" = 128 | 256 forces one of the two -- the tests run every shape through both)
  const int forced = (int)option(OPT_FX_ROWS);
  // fp32-NCL output of at most 128 channels (the pre-VQ convolution and the data gradient that leaves the decoder): a
  // 128-channel m-tile on 128-row tiles -- no MFMA spent on padding channels (option "fx_narrow" = 0 switches it off)
  const bool narrow = !dbg_env && y_ncl && M <= 128 && option(OPT_FX_NARROW) != 0;
  const bool half = narrow || (!dbg_env && (forced == 128 || (forced != 256 && a.b.rtiles * a.b.mtiles < 192)));
  if (half) a.b.rtiles = (int)(rows / 128);
  const dim3 grid(a.b.rtiles * a.b.mtiles), block(512);
#ifdef ALVQ_DEBUG_KERNELS
  if (dbg_env && y) {
    static unsigned long long* stamps = nullptr;
    if ((dbg_env & (256 | 512)) && !stamps) (void)hipMalloc(&stamps, 4096 * 4 * sizeof(unsigned long long));
    a.stamps = stamps;
    if (grid.x > 4096) a.dbg &= ~(256 | 512);
    if (KW == 3 && (dbg_env & 16)) hipLaunchKernelGGL((conv1d_f16mx_kernel<0, 3, 2>), grid, block, ConvRings::LDS, s, a);
    else if (KW == 3 && (dbg_env & 32)) hipLaunchKernelGGL((conv1d_f16mx_kernel<0, 3, 3>), grid, block, ConvRings::LDS, s, a);
    else if (KW == 3) hipLaunchKernelGGL((conv1d_f16mx_kernel<0, 3, 1>), grid, block, ConvRings::LDS, s, a);
    else hipLaunchKernelGGL((conv1d_f16mx_kernel<0, 1, 1>), grid, block, ConvRings::LDS, s, a);
    if (a.dbg & (256 | 512)) {     // phase durations of this launch (means over its workgroups; first / last round by start time)
      (void)hipStreamSynchronize(s);
      static unsigned long long h[4096 * 4];
      (void)hipMemcpy(h, stamps, grid.x * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
      unsigned long long t0 = ~0ull, t1 = 0;
      for (unsigned i = 0; i < grid.x; ++i) { if (h[4 * i] < t0) t0 = h[4 * i]; if (h[4 * i + 3] > t1) t1 = h[4 * i + 3]; }
      double pro[2] = {0, 0}, mainl[2] = {0, 0}, epi[2] = {0, 0}, start[2] = {0, 0}; int cnt[2] = {0, 0};
      for (unsigned i = 0; i < grid.x; ++i) {
        const int rnd = (h[4 * i] - t0) * 4 > (t1 - t0) ? 1 : 0;     // started in the first quarter of the launch or later
        pro[rnd] += h[4 * i + 1] - h[4 * i]; mainl[rnd] += h[4 * i + 2] - h[4 * i + 1]; epi[rnd] += h[4 * i + 3] - h[4 * i + 2];
        start[rnd] += h[4 * i] - t0; ++cnt[rnd];
      }
      for (int r = 0; r < 2; ++r)
        if (cnt[r])
          fprintf(stderr, "[fx stamps] KW=%d M=%d C=%d round %d: %d workgroups, start +%.1f us, staging %.2f us, main loop %.2f us, epilogue %.2f us\n",
                  KW, M, C, r, cnt[r], start[r] / cnt[r] / 100.0, pro[r] / cnt[r] / 100.0, mainl[r] / cnt[r] / 100.0, epi[r] / cnt[r] / 100.0);
      fprintf(stderr, "[fx stamps] launch span %.1f us\n", (t1 - t0) / 100.0);
    }
    return check_launch("alvq_conv1d_f16mx(dbg)");
  }
#endif
  // one of the three operand sets of a train step's forward launches, on whole m-tiles: the kernel compiled for that set
  // (option "fx_epi" = 0 sends every launch to the general epilogue)
  int epi = 0;
  if (y && !skip2 && !mask && !mask_bits && !post && a.b.Mop % ConvRings::M == 0 && option(OPT_FX_EPI) != 0)
    epi = bias ? (skip1 ? 0 : 2) : (skip1 ? 3 : 1);
  return table.launch(fx_slot(y ? 0 : 1, KW, half ? 1 : 2, narrow ? 2 : 4, epi), grid, block, s, "alvq_conv1d_f16mx", a);
}
