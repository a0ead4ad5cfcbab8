// Split-bf16 ("bf16x3") convolution and weight-gradient: fp32-grade results on the bf16 matrix cores.
//
// gfx950 has no TF32/xf32 MFMA and its exact-fp32 MFMA runs at 1/16 of the bf16 rate.  Here every fp32 value v is
// carried as two bf16 planes, hi = bf16(v) and lo = bf16(v - hi) (|v - hi - lo| <= 2^-18 |v|), and every product
// is evaluated as  hi*hi + hi*lo + lo*hi  (three bf16 MFMAs, fp32 accumulation; the lo*lo term, <= 2^-18 relative,
// is dropped).  bf16 x bf16 products are exact in fp32, so the result differs from an fp32 computation only by
// ~1e-5 relative -- well inside the 1e-3 parity bar -- at one third of the bf16 MFMA rate, i.e. ~5x the exact-fp32
// MFMA peak.  Storage cost equals fp32 (two bf16 planes per tensor).
//
// Layout: the NLC-padded matrix of include/alvq.h, with the lo plane stored right after the hi plane (guard rows
// included): lo = hi + alvq_nlc_plane_bytes(B, L, C).  Packed weights likewise (lo image after the hi image).
//
// Kernels: same tiling as conv1d_bf16_v2 / conv1d_wgrad_bf16_v2 (256x256 tile, 8 waves; 128x128x3-tap tile for the
// weight-gradient) with a 2-stage LDS-DMA ring (a K-tile now carries 4 slabs and 96 MFMAs per wave, so one
// iteration of look-ahead already gives the DMA ~3000 cycles).
#include <stdlib.h>

#include "alvq_common.h"
#include "bf16_common.h"
#include "conv_tile.h"
#include "nlc_host.h"
#include "wgrad_bias_reduce.h"
#include "wgrad_reduce.h"
#include "wgrad_tile.h"

namespace alvq {

struct ConvX3Args {
  ConvBArgs b;          // hi planes (and everything shared)
  long x_plane, wp_plane, y_plane;   // element offsets (u16) from a hi pointer to its lo plane
};

__device__ __forceinline__ void split2(float v, u16& hi, u16& lo) {
  hi = f2bf(v);
  lo = f2bf(v - bf2f(hi));
}

// 8 consecutive channels of one row -> packed hi and lo words (hardware bf16 rounding)
__device__ __forceinline__ void split_pack8(const float (&v)[8], u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    hi[e] = f2bf_pk(v[2 * e], v[2 * e + 1]);
    lo[e] = f2bf_pk(v[2 * e] - __uint_as_float(hi[e] << 16), v[2 * e + 1] - __uint_as_float(hi[e] & 0xffff0000u));
  }
}

// Register-direct epilogue of one wave's 128 (m) x 64 (rows) block, split-bf16 flavour of wave_epilogue_bf16
// (conv_tile.h): v_permlane16_swap gives every lane 8 consecutive channels, 16-byte loads and stores.  Written,
// like that one, for few VALU instructions per value: a row block's offset is formed once, the skip / mask operands of
// the whole row block are requested before the first group is finished, nothing is computed for absent operands, gap
// rows are zeroed by a select on the packed words inside a wave-uniform branch.
template <int NNI>
__device__ __forceinline__ void wave_epilogue_x3(const ConvX3Args& ax, const f32x4 (&acc)[8][NNI], int m0, int r0, int li,
                                                 int kq, int wm0, int wn0) {
  const ConvBArgs& a = ax.b;
  const int Lp1 = a.L + 1, ndata = a.B * Lp1;
  const int mb0 = m0 + wm0 + (kq & 1) * 16 + (kq >> 1) * 8;
  const long pl = ax.y_plane;
#pragma unroll
  for (int ni = 0; ni < NNI; ++ni) {
    const int row = r0 + wn0 + ni * 16 + li;
    int b, l;
    const bool ok = row_valid(row, Lp1, ndata, &b, &l);
    const bool gaps = !__all(ok);
    const long o0 = (long)row * a.Mop + mb0;
    u16x8 s1h[4], s1l[4], mk[4];
#pragma unroll
    for (int mp = 0; mp < 8; mp += 2) {
      if (m0 + wm0 + mp * 16 >= a.Mop) continue;
      if (a.skip1) {
        s1h[mp / 2] = *(const u16x8*)(a.skip1 + o0 + mp * 16);
        s1l[mp / 2] = *(const u16x8*)(a.skip1 + pl + o0 + mp * 16);
      }
      if (a.mask) mk[mp / 2] = *(const u16x8*)(a.mask + o0 + mp * 16);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mp = 0; mp < 8; mp += 2) {
      if (m0 + wm0 + mp * 16 >= a.Mop) continue;
      const long o = o0 + mp * 16;
      const int mb = mb0 + mp * 16;
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[mp][ni][e]), __float_as_uint(acc[mp + 1][ni][e]),
                                                         false, false);
        v[e] = __uint_as_float(r[0]);
        v[e + 4] = __uint_as_float(r[1]);
      }
      if (a.bias) {
        if (m0 + wm0 + mp * 16 + 32 <= a.M) {
          const f32x4 b0 = *(const f32x4*)(a.bias + mb), b1 = *(const f32x4*)(a.bias + mb + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] += b0[e];
            v[4 + e] += b1[e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += (mb + e < a.M) ? a.bias[mb + e] : 0.f;
        }
      }
      if (a.skip1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bf2f(s1h[mp / 2][e]) + bf2f(s1l[mp / 2][e]);
      }
      if (a.skip2) {
        const u16x8 sh = *(const u16x8*)(a.skip2 + o), sl = *(const u16x8*)(a.skip2 + pl + o);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bf2f(sh[e]) + bf2f(sl[e]);
      }
      if (a.relu & 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      if (a.mask) {   // sign of a split value is the sign of its hi plane
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = bf2f(mk[mp / 2][e]) > 0.f ? v[e] : 0.f;
      }
      u32x4 hi, lo;
      split_pack8(v, hi, lo);
      if (gaps) {                                           // gap / tail rows stay zero in both planes
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          hi[e] = ok ? hi[e] : 0u;
          lo[e] = ok ? lo[e] : 0u;
        }
      }
      *(u32x4*)(a.y + o) = hi;
      *(u32x4*)(a.y + pl + o) = lo;
      if (a.y2) {
        const u16x8 ph = *(const u16x8*)(a.post + o), pq = *(const u16x8*)(a.post + pl + o);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bf2f(ph[e]) + bf2f(pq[e]);
        split_pack8(v, hi, lo);
        if (gaps) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            hi[e] = ok ? hi[e] : 0u;
            lo[e] = ok ? lo[e] : 0u;
          }
        }
        *(u32x4*)(a.y2 + o) = hi;
        *(u32x4*)(a.y2 + pl + o) = lo;
      }
    }
  }
}

// wave_epilogue_x3 for the two operand sets the forward launches of a train step are made of, on a wave block that lies
// inside Mop: OPS == 1 skip1 alone, OPS == 2 bias alone (ReLU either way, at run time: it loads nothing).  Same values
// combined in the same order and stored to the same addresses, but no wait on a load issued behind one of the wave's own
// stores (gfx950 counts vector loads and stores in ONE counter and retires it in issue order: such a wait also waits for the
// store's write acknowledgement), and the set is a template argument because behind a branch on an operand's presence the
// compiler cannot count the loads in flight and waits for all of them, stores included.
//  * skip1 is 4 bytes per element: all NNI row blocks at once would be 128 registers next to the 128 accumulators.  It goes
//    one row block ahead through ONE 32-register buffer: block ni + 1 is requested after block ni has been packed (32
//    registers of hi / lo words, while its 32 accumulators die) and before block ni is stored.
//  * the bias is added into the accumulators in front of everything: lane (li, kq) of fragment mi holds channels
//    mi*16 + kq*4 .. +3 of every row block, so a fragment's bias is one 16-byte load for all row blocks, and acc + bias is the
//    same float on either side of the lane swap.  The loop then loads nothing.
template <int NNI, int OPS>
__device__ __forceinline__ void wave_epilogue_x3_ordered(const ConvX3Args& ax, f32x4 (&acc)[8][NNI], int m0, int r0, int li,
                                                         int kq, int wm0, int wn0) {
  const ConvBArgs& a = ax.b;
  const int Lp1 = a.L + 1, ndata = a.B * Lp1;
  const int mb0 = m0 + wm0 + (kq & 1) * 16 + (kq >> 1) * 8;
  const long pl = ax.y_plane;
  const long o00 = (long)(r0 + wn0 + li) * a.Mop + mb0, oblk = (long)16 * a.Mop;
  u16x8 s1h[4], s1l[4];
  auto request = [&](int ni) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      s1h[p] = *(const u16x8*)(a.skip1 + o00 + ni * oblk + p * 32);
      s1l[p] = *(const u16x8*)(a.skip1 + pl + o00 + ni * oblk + p * 32);
    }
  };
  if (OPS == 1) request(0);
  if (OPS == 2) {
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
      const int c0 = m0 + wm0 + mi * 16 + kq * 4;
      f32x4 bv;
      if (m0 + wm0 + (mi & ~1) * 16 + 32 <= a.M) {     // the pair lies inside M
        bv = *(const f32x4*)(a.bias + c0);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = (c0 + e < a.M) ? a.bias[c0 + e] : 0.f;
      }
#pragma unroll
      for (int ni = 0; ni < NNI; ++ni)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[mi][ni][e] += bv[e];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int ni = 0; ni < NNI; ++ni) {
    int b, l;
    const bool ok = row_valid(r0 + wn0 + ni * 16 + li, Lp1, ndata, &b, &l);
    const bool gaps = !__all(ok);
    u32x4 hi[4], lo[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][ni][e]), __float_as_uint(acc[2 * p + 1][ni][e]),
                                                         false, false);
        v[e] = __uint_as_float(r[0]);
        v[e + 4] = __uint_as_float(r[1]);
      }
      if (OPS == 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bf2f(s1h[p][e]) + bf2f(s1l[p][e]);
      }
      if (a.relu & 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      split_pack8(v, hi[p], lo[p]);
      if (gaps) {                                           // gap / tail rows stay zero in both planes
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          hi[p][e] = ok ? hi[p][e] : 0u;
          lo[p][e] = ok ? lo[p][e] : 0u;
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (OPS == 1 && ni + 1 < NNI) request(ni + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      *(u32x4*)(a.y + o00 + ni * oblk + p * 32) = hi[p];
      *(u32x4*)(a.y + pl + o00 + ni * oblk + p * 32) = lo[p];
    }
  }
}

// Main kernel.  A K-tile = (32 channels, one tap), staged through the two rings of conv_tile.h (ConvRings: W hi, W lo per
// K-tile; X hi, X lo per chunk).  Per wave a K-tile is three phases of 32 MFMAs on the same 8 x 4 accumulators:
//   phase 1  hi*hi : A0 = W hi fragments, BX = X hi        | meanwhile: read X lo -> BY, first half of W lo -> A1
//   phase 2  hi*lo : A0, BY                                 | meanwhile: second half of W lo -> A1
//            s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier      <- K-tile t+1 has landed; every read of this K-tile is done
//   phase 3  lo*hi : A1, BX                                 | meanwhile: DMA of K-tile t+2's weights into THIS weight
//                                                             stage (and, on taps 0 / 1, of the next chunk's activation
//                                                             planes); the hi fragments of K-tile t+1 -> A0 and BY
// so the barrier falls between phases whose operands are already in registers: no fragment read is ever exposed
// behind it, every LDS read has at least half a phase (16 MFMAs) to return, and the X fragment sets swap roles from
// one K-tile to the next (BX <-> BY).  96 fragment VGPRs + 128 accumulators.  MFMAs are tied inline asm (hipcc does
// not tie the builtin's destination to its C operand and then shuffles the accumulators through spare registers it
// does not have here).

// NNI: 16-row fragments per wave.  4 = the 256 x 256 tile (a wave owns 128 channels x 64 rows); 2 (round 4) = a 128-channel
// m-tile x 256 rows: every wave owns all 128 channels x 32 rows, waves 0-3 stage the 128 weight rows.  For layers of at most
// 128 output channels -- the pre-VQ convolution's 256-wide tile spent half of its MFMAs (171 us of the default mode's step) on
// padding channels -- and for problems with too few 256 x 256 tiles to cover the chip (the RIR config's 1024-channel layers:
// 104 tiles on 256 CUs -> 208 workgroups of half the work).  1 = 128 channels x 128 rows (a wave owns 128 x 16; waves 0-3 stage
// the activation rows as well): twice the workgroups again for the launches that still leave CUs idle (the speech pre-VQ
// convolution: 126 -> 251 workgroups).  Same K order per output: results are bit-identical.
template <int OUT, int KW, int NNI = 4>
__global__ __launch_bounds__(512, 2) void conv1d_bf16x3_kernel(ConvX3Args ax) {
  static_assert(NNI == 4 || NNI == 2 || NNI == 1, "4, 2 or 1 row fragments per wave");
  typedef ConvRings G;
  constexpr int MT = NNI == 4 ? G::M : 128;
  constexpr int RT = NNI == 1 ? 128 : G::R;
  const ConvBArgs& a = ax.b;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, kq = lane >> 4;
  const int wm0 = NNI == 4 ? (wave >> 2) * 128 : 0, wn0 = NNI == 4 ? (wave & 3) * 64 : wave * 16 * NNI;

  const ConvTileOrigin o = conv_tile_origin<MT, RT>(a);
  const int m0 = o.m0, r0 = o.r0;
  const int Cp = a.Cp;
  // ---- DMA sources (ConvRingStager, conv_tile.h, says what each is): plane 0 = hi, plane 1 = lo
  const int srow = slab64_lane(lane).row;
  const unsigned lane_off = slab64_lane_off(lane, Cp);
  const long tap_w = (long)a.Mp128 * Cp * 2;
  const long row16 = (long)Cp * 32;
  const long wpl = ax.wp_plane * 2, xpl = ax.x_plane * 2;
  const char* const wb = (const char*)(a.wp + ((long)m0 + wave * 32) * Cp);
  const char* const xb = (const char*)(a.x + ((long)r0 - (KW - 1) / 2 + wave * 32) * Cp);
  const ConvRingStager<KW, MT, RT, false> st(wave, srow, lane_off, tap_w, row16, wpl, xpl, wb, xb);

  // ---- fragment reads (plane 0 = hi, 1 = lo); activations of tap t: slab row = local row + t
  const int loffA = slab64_frag16(li, kq, 0);
  int loffB[KW];
#pragma unroll
  for (int t = 0; t < KW; ++t) loffB[t] = slab64_frag16(li, kq, t);
  const unsigned char* const abase = lds + wm0 * 64 + loffA;
  const unsigned char* const bbase = lds + G::XBASE + wn0 * 64;
  bf16x8_t fa0[8], fa1[8], fb0[NNI], fb1[NNI];
#define X3_RDA(DST, HALF, WS, PLANE)                                                               \
  {                                                                                                \
    const unsigned char* pa_ = abase + (WS) * G::WSTAGE + (PLANE) * G::SLAB;                       \
    _Pragma("unroll") for (int mi = (HALF) * 4; mi < (HALF) * 4 + 4; ++mi) DST[mi] = *(const bf16x8_t*)(pa_ + mi * 1024); \
  }
#define X3_RDB(DST, XS, TAP, PLANE)                                                                \
  {                                                                                                \
    const unsigned char* pb_ = bbase + (XS) * G::XSTAGE + (PLANE) * G::XSLAB + loffB[TAP];         \
    _Pragma("unroll") for (int ni = 0; ni < NNI; ++ni) DST[ni] = *(const bf16x8_t*)(pb_ + ni * 1024); \
  }

  f32x4 acc[8][NNI];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NNI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#define X3_MM(A, B, HALF)                                                                          \
  _Pragma("unroll") for (int mi = (HALF) * 4; mi < (HALF) * 4 + 4; ++mi)                           \
  _Pragma("unroll") for (int ni = 0; ni < NNI; ++ni)                                               \
      asm("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[mi][ni]) : "v"(A[mi]), "v"(B[ni]));
#define X3_SB __builtin_amdgcn_sched_barrier(0);

  const int nch = Cp / G::K;        // chunks; even (Cp % 64 == 0)
  const int n = nch * KW;           // K-tiles
  const bool early = wave < 4;      // the two waves of a SIMD issue their DMA at different points of phase 3

  // ---- prologue: chunk 0's activation slabs, K-tiles 0 and 1 (and, for width 1, chunk 1's slabs) staged; hi fragments
  // of K-tile 0 in A0 / fb0
  st.prologue(lds, n, nch);
  X3_RDA(fa0, 0, 0, 0)
  X3_RDA(fa0, 1, 0, 0)
  X3_RDB(fb0, 0, 0, 0)

  // one K-tile: weights in stage WS, activations in stage XS at tap TAP, X hi in BX; BY receives X lo and, in phase 3,
  // the next K-tile's X hi (NWS, NXS, NTAP).  DMA_ = what this K-tile stages right behind its barrier.
#define X3_TILE(WS, XS, TAP, NWS, NXS, NTAP, BX, BY, DMA_)                                         \
  X3_MM(fa0, BX, 0) X3_SB X3_RDB(BY, XS, TAP, 1) X3_SB                                             \
  X3_MM(fa0, BX, 1) X3_SB X3_RDA(fa1, 0, WS, 1) X3_SB                                              \
  X3_MM(fa0, BY, 0) X3_SB X3_RDA(fa1, 1, WS, 1) X3_SB                                              \
  X3_MM(fa0, BY, 1) X3_SB                                                                          \
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                      \
  __builtin_amdgcn_s_barrier();                                                                    \
  if (early) { DMA_ }                                                                              \
  X3_MM(fa1, BX, 0) X3_SB X3_RDA(fa0, 0, NWS, 0) X3_RDB(BY, NXS, NTAP, 0) X3_SB                    \
  if (!early) { DMA_ }                                                                             \
  X3_MM(fa1, BX, 1) X3_SB X3_RDA(fa0, 1, NWS, 0) X3_SB

  if (KW == 3) {
    // two chunks (six K-tiles) per iteration: every stage index and the BX / BY roles are constants
    for (int c = 0; c < nch; c += 2) {
      const int t = 3 * c;
      X3_TILE(0, 0, 0, 1, 0, 1, fb0, fb1, if (t + 2 < n) st.issueW(lds, t + 2); if (c + 1 < nch) st.issueX(lds, c + 1, 0);)
      X3_TILE(1, 0, 1, 0, 0, 2, fb1, fb0, if (t + 3 < n) st.issueW(lds, t + 3); if (c + 1 < nch) st.issueX(lds, c + 1, 1);)
      X3_TILE(0, 0, 2, 1, 1, 0, fb0, fb1, if (t + 4 < n) st.issueW(lds, t + 4);)
      X3_TILE(1, 1, 0, 0, 1, 1, fb1, fb0, if (t + 5 < n) st.issueW(lds, t + 5); if (c + 2 < nch) st.issueX(lds, c + 2, 0);)
      X3_TILE(0, 1, 1, 1, 1, 2, fb0, fb1, if (t + 6 < n) st.issueW(lds, t + 6); if (c + 2 < nch) st.issueX(lds, c + 2, 1);)
      X3_TILE(1, 1, 2, 0, 0, 0, fb1, fb0, if (t + 7 < n) st.issueW(lds, t + 7);)
    }
  } else {
    for (int t = 0; t < n; t += 2) {
      X3_TILE(0, 0, 0, 1, 1, 0, fb0, fb1, if (t + 2 < n) { st.issueW(lds, t + 2); st.issueX(lds, t + 2, 0); st.issueX(lds, t + 2, 1); })
      X3_TILE(1, 1, 0, 0, 0, 0, fb1, fb0, if (t + 3 < n) { st.issueW(lds, t + 3); st.issueX(lds, t + 3, 0); st.issueX(lds, t + 3, 1); })
    }
  }
#undef X3_TILE
#undef X3_SB
#undef X3_MM
#undef X3_RDB
#undef X3_RDA
  // the compiler's hazard recogniser does not see inside the asm MFMAs: cover the MFMA-result -> VALU-read wait
  // states by hand before the epilogue touches the accumulators
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");

  if constexpr (OUT == 0) {   // bf16 hi + lo planes, straight from the accumulators
    const bool plain = !a.skip2 && !a.mask && !a.y2 && m0 + wm0 + 128 <= a.Mop;
    if (plain && a.skip1 && !a.bias) wave_epilogue_x3_ordered<NNI, 1>(ax, acc, m0, r0, li, kq, wm0, wn0);
    else if (plain && a.bias && !a.skip1) wave_epilogue_x3_ordered<NNI, 2>(ax, acc, m0, r0, li, kq, wm0, wn0);
    else wave_epilogue_x3(ax, acc, m0, r0, li, kq, wm0, wn0);
    return;
  }
  __syncthreads();   // the C slab overlays the stages: the trailing fragment reads of every wave must be done
  // ---- OUT == 1: 64-row slabs, each written by the waves that own rows of it (four of them; two / four in the narrow tiles)
  conv_store_ncl<false, MT, RT>(a, lds, m0, r0, tid, nullptr, [&](float* Cs, int slab) {
    if ((wn0 >> 6) == slab) store_frags16<C_SLAB_STRIDE>(Cs, acc, li, kq, wm0, wn0 & 63);
  });
}

// ------------------------------------------------------------------------------------------- weight-gradient
struct WgradX3Args {
  // Up to WGRAD_MAXSEG (dy, x) pairs of identical shape whose products are summed into ONE dW (the R uses of a shared
  // residual weight): virtual row v = seg * total_rows + r, as in the bf16 and f16mx weight gradients.
  const u16* dy[WGRAD_MAXSEG];
  const u16* x[WGRAD_MAXSEG];
  int nseg;
  float* partial;
  float* bias_partial;   // [splits][Mp] column sums of dY (the bias gradient), or null
  long dy_plane, x_plane;
  int Mp, Cp, M, C;
  int mtiles, ctiles, splits, chunks_per_split, total_rows;
};

template <int KW, int NCF>
__global__ __launch_bounds__(512, 2) void conv1d_wgrad_bf16x3_kernel(WgradX3Args a) {
  constexpr int MT = 128, CT = 4 * NCF * 16;
  typedef WgradSlabs<KW, MT, CT, 2> Slabs;                 // a stage: dY_hi, dY_lo, X_hi, X_lo
  constexpr int YRB = Slabs::YRB, XRB = Slabs::XRB, YBYTES = Slabs::YBYTES, XBYTES = Slabs::XBYTES;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave >> 2) * 64, wc0 = (wave & 3) * NCF * 16;
  const WgradWork w = wgrad_work<MT, CT>(a);
  const int n = w.n;
  WgradStager<WgradX3Args, KW, MT, CT, 2, LdsDmaAsm> st(a, wave, lane, w);

  int ybase, xbase[KW], yseg[4], xseg[NCF], xline[NCF];
  wgrad_frag16_bases<KW, NCF, YRB, XRB>(lane, wm0, wc0, ybase, xbase, yseg, xseg, xline);

  f32x4 acc[KW][4][NCF];
#pragma unroll
  for (int t = 0; t < KW; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NCF; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // bias gradient = column sums of dY (hi + lo): the workgroups of c-tile 0 multiply their dY fragments by an all-ones
  // operand as well (one wave per 64 m), instead of a separate pass re-reading dY
  const bool do_bias = a.bias_partial != nullptr && w.c0 == 0 && (wave & 3) == 0;
  f32x4 accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  typedef short s16x8_t __attribute__((ext_vector_type(8)));
  const s16x8_t ones_raw = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  bf16x8_t ones = __builtin_bit_cast(bf16x8_t, ones_raw);
  // Opaque from here on: a known constant would be re-materialised by VALU moves right in front of each use, and the
  // compiler inserts the VALU-write -> MFMA-read wait states only for MFMAs it can see (the ones below are inline asm;
  // observed: wrong bias sums in the KW = 1 instantiation, where register pressure triggers the re-materialisation).
  asm volatile("" : "+v"(ones));

  // Fragment halves as the transposing reads return them.  Same phase structure as the convolution above: a K-tile
  // (32 rows) is hi*hi, hi*lo, [barrier], lo*hi; the barrier sits between phases whose operands are in registers,
  // the lo fragments are read during phase 1, the next K-tile's hi fragments during phase 3 (A hi and the X set that
  // phase 2 has finished with are dead by then), and the two X fragment sets swap roles from one K-tile to the next.
  bf16x8_t ah[4], al[4], b0[KW][NCF], b1[KW][NCF];
#define WX_RDA(DST, STAGE, PLANE, MI) \
  DST[MI] = wgrad_tr16_pair<bf16x8_t>(lds + ((STAGE) * STAGE_B + (PLANE) * YBYTES + (ybase ^ yseg[MI])), YRB);
#define WX_RDB(DST, STAGE, PLANE, TP, CF)                                                                                      \
  DST[TP][CF] = wgrad_tr16_pair<bf16x8_t>(                                                                                     \
      lds + ((STAGE) * STAGE_B + 2 * YBYTES + (PLANE) * XBYTES + ((xbase[TP] ^ xseg[CF]) + xline[CF])), XRB);
  // MFMAs of one m-fragment against every (tap, c-fragment) of an X set (tied asm: see the convolution kernel)
#define WX_MM(A, B, MI)                                                                                    \
  _Pragma("unroll") for (int tp = 0; tp < KW; ++tp)                                                        \
  _Pragma("unroll") for (int cf = 0; cf < NCF; ++cf)                                                       \
      asm("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[tp][MI][cf]) : "v"(A[MI]), "v"(B[tp][cf]));
  // the bias MFMAs exist only in the loop the c-tile-0 waves run: a per-use `if (do_bias)` around inline asm makes hipcc
  // carry copies of the accumulators across every branch (31 v_mov_b64 each, in every wave)
#define WX_BIAS_ON(A, MI) asm("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(accb[MI]) : "v"(A[MI]), "v"(ones));
#define WX_BIAS_OFF(A, MI)
#define WX_SB __builtin_amdgcn_sched_barrier(0);
  constexpr int STAGE_B = Slabs::STAGE;

  // one K-tile in stage S; BX = X hi fragments (already in registers), BY receives X lo, then the next tile's X hi
#define WX_TILE(S, BX, BY, MORE, WX_BIAS)                                                                         \
  /* phase 1: hi*hi; meanwhile X lo -> BY and dY lo -> al */                                               \
  WX_MM(ah, BX, 0) WX_BIAS(ah, 0) WX_SB                                                                    \
  _Pragma("unroll") for (int tp = 0; tp < KW; ++tp) _Pragma("unroll") for (int cf = 0; cf < NCF; ++cf) WX_RDB(BY, S, 1, tp, cf) \
  WX_SB WX_MM(ah, BX, 1) WX_BIAS(ah, 1) WX_SB                                                              \
  WX_RDA(al, S, 1, 0) WX_RDA(al, S, 1, 1) WX_RDA(al, S, 1, 2) WX_RDA(al, S, 1, 3)                          \
  WX_SB WX_MM(ah, BX, 2) WX_BIAS(ah, 2) WX_MM(ah, BX, 3) WX_BIAS(ah, 3) WX_SB                              \
  /* phase 2: hi*lo */                                                                                     \
  WX_MM(ah, BY, 0) WX_MM(ah, BY, 1) WX_MM(ah, BY, 2) WX_MM(ah, BY, 3) WX_SB                                \
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                              \
  __builtin_amdgcn_s_barrier();                                                                            \
  /* phase 3: lo*hi; meanwhile the DMA of K-tile t+2 into this stage and the next tile's hi fragments */   \
  if (MORE) st.issue(lds, S);                                                                              \
  WX_MM(al, BX, 0) WX_BIAS(al, 0) WX_SB                                                                    \
  WX_RDA(ah, (S) ^ 1, 0, 0) WX_RDA(ah, (S) ^ 1, 0, 1) WX_RDA(ah, (S) ^ 1, 0, 2) WX_RDA(ah, (S) ^ 1, 0, 3)  \
  WX_SB WX_MM(al, BX, 1) WX_BIAS(al, 1) WX_SB                                                              \
  _Pragma("unroll") for (int tp = 0; tp < KW; ++tp) _Pragma("unroll") for (int cf = 0; cf < NCF; ++cf) WX_RDB(BY, (S) ^ 1, 0, tp, cf) \
  WX_SB WX_MM(al, BX, 2) WX_BIAS(al, 2) WX_MM(al, BX, 3) WX_BIAS(al, 3) WX_SB

  if (n > 0) {
    st.issue(lds, 0);
    if (n > 1) st.issue(lds, 1);
    st.wait_keep(n > 1 ? 1 : 0);   // K-tile 0 landed; K-tile 1's pieces (this wave's count) may stay in flight
    __builtin_amdgcn_s_barrier();
    WX_RDA(ah, 0, 0, 0) WX_RDA(ah, 0, 0, 1) WX_RDA(ah, 0, 0, 2) WX_RDA(ah, 0, 0, 3)
#pragma unroll
    for (int tp = 0; tp < KW; ++tp)
#pragma unroll
      for (int cf = 0; cf < NCF; ++cf) WX_RDB(b0, 0, 0, tp, cf)
    if (do_bias) {
      for (int t = 0; t < n; t += 2) {
        WX_TILE(0, b0, b1, t + 2 < n, WX_BIAS_ON)
        WX_TILE(1, b1, b0, t + 3 < n, WX_BIAS_ON)
      }
    } else {
      for (int t = 0; t < n; t += 2) {
        WX_TILE(0, b0, b1, t + 2 < n, WX_BIAS_OFF)
        WX_TILE(1, b1, b0, t + 3 < n, WX_BIAS_OFF)
      }
    }
    // the compiler's hazard recogniser does not see inside the asm MFMAs: cover the MFMA-result -> VALU-read wait
    // states by hand before the accumulators are stored
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  }
#undef WX_TILE
#undef WX_SB
#undef WX_BIAS_ON
#undef WX_BIAS_OFF
#undef WX_MM
#undef WX_RDB
#undef WX_RDA

  wgrad_store16<KW, NCF>(a, w, lane, wm0, wc0, acc, do_bias, accb);
}

__global__ __launch_bounds__(256) void ncl_to_nlc_x3_kernel(const float* x, u16* y, long plane, int B, int C, int L, int Cp,
                                                            int rows_total) {
  __shared__ float tile[32][33];
  const int ct = Cp / 32;
  const int r0 = (blockIdx.x / ct) * 32, c0 = (blockIdx.x % ct) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int Lp1 = L + 1, ndata = B * Lp1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, row = r0 + tx;
    int b, l;
    const bool ok = row_valid(row, Lp1, ndata, &b, &l) && c < C;
    tile[ty + 8 * i][tx] = ok ? x[((long)b * C + c) * L + l] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = r0 + ty + 8 * i, c = c0 + tx;
    if (row < rows_total) {
      u16 hi, lo;
      split2(tile[tx][ty + 8 * i], hi, lo);
      y[(long)row * Cp + c] = hi;
      y[plane + (long)row * Cp + c] = lo;
    }
  }
}

__global__ __launch_bounds__(256) void nlc_to_ncl_x3_kernel(const u16* x, long plane, float* y, int B, int C, int L, int Cp,
                                                            int rows_total) {
  __shared__ float tile[32][33];
  const int ct = Cp / 32;
  const int r0 = (blockIdx.x / ct) * 32, c0 = (blockIdx.x % ct) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int Lp1 = L + 1, ndata = B * Lp1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = r0 + ty + 8 * i, c = c0 + tx;
    tile[ty + 8 * i][tx] = row < rows_total ? bf2f(x[(long)row * Cp + c]) + bf2f(x[plane + (long)row * Cp + c]) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, row = r0 + tx;
    int b, l;
    if (row_valid(row, Lp1, ndata, &b, &l) && c < C) y[((long)b * C + c) * L + l] = tile[tx][ty + 8 * i];
  }
}

// out = t > 0 ? dy : 0 on both planes (the sign of a split value is the sign of its hi plane)
__global__ __launch_bounds__(256) void relu_mask_x3_kernel(const u16* dy, const u16* t, u16* out, long plane8, long n8) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n8; e += (long)gridDim.x * 256) {
    const u16x8 dh = ((const u16x8*)dy)[e], dl = ((const u16x8*)dy)[plane8 + e], m = ((const u16x8*)t)[e];
    u16x8 oh, ol;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool keep = bf2f(m[i]) > 0.f;
      oh[i] = keep ? dh[i] : (u16)0;
      ol[i] = keep ? dl[i] : (u16)0;
    }
    ((u16x8*)out)[e] = oh;
    ((u16x8*)out)[plane8 + e] = ol;
  }
}

template <int KW, int NCF>
static constexpr int wgrad_x3_lds() {
  return 2 * WgradSlabs<KW, 128, 4 * NCF * 16, 2>::STAGE;
}

// tile of a launch: 128 m x {128 c x 3 taps | 256 c}
static WgradTile wgrad_x3_tile(int KW) { return {128, KW == 3 ? 128 : 256}; }

constexpr int X3_BIAS_SPLITS = 64;     // upper bound of the split count (wgrad_split_plan)

}  // namespace alvq

using namespace alvq;

extern "C" int64_t alvq_nlc_plane_bytes(int B, int L, int C) {
  return (B <= 0 || L <= 0 || C <= 0) ? -1 : nlc_plane_elems(B, L, C) * 2;
}

extern "C" int alvq_pack_weight_bf16x3(const float* w, void* wp, int M, int C, int KW, int w_layout, void* stream) {
  const alvq_pack_desc d{w, wp, M, C, KW, w_layout};     // one-descriptor batch, hi + lo images (pack_weights.hip)
  return alvq_pack_weights_bf16_batch(&d, 1, 2, stream);
}

extern "C" int alvq_ncl_to_nlc_bf16x3(const float* x, void* y, int B, int C, int L, void* stream) {
  if (int rc = check_nlc_dims("alvq_ncl_to_nlc_bf16x3", x && y, B, C, L)) return rc;
  const NlcDims d(B, C, L);
  hipLaunchKernelGGL(ncl_to_nlc_x3_kernel, d.grid32(), dim3(256), 0, (hipStream_t)stream, x, (u16*)y, d.plane, B, C, L, d.Cp, d.rows);
  return check_launch("alvq_ncl_to_nlc_bf16x3");
}

extern "C" int alvq_nlc_to_ncl_bf16x3(const void* x, float* y, int B, int C, int L, void* stream) {
  if (int rc = check_nlc_dims("alvq_nlc_to_ncl_bf16x3", x && y, B, C, L)) return rc;
  const NlcDims d(B, C, L);
  hipLaunchKernelGGL(nlc_to_ncl_x3_kernel, d.grid32(), dim3(256), 0, (hipStream_t)stream, (const u16*)x, d.plane, y, B, C, L, d.Cp,
                     d.rows);
  return check_launch("alvq_nlc_to_ncl_bf16x3");
}

extern "C" int alvq_relu_mask_bf16x3(const void* dy, const void* t, void* out, int B, int C, int L, void* stream) {
  if (int rc = check_nlc_dims("alvq_relu_mask_bf16x3", dy && t && out, B, C, L)) return rc;
  const NlcDims d(B, C, L);
  const long n = (long)d.rows * d.Cp;
  long g = (n / 8 + 1023) / 1024;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(relu_mask_x3_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, (const u16*)dy, (const u16*)t,
                     (u16*)out, d.plane / 8, n / 8);
  return check_launch("alvq_relu_mask_bf16x3");
}

// conv1d_bf16x3_kernel<OUT, KW, NNI> sits at x3_slot(OUT, KW, NNI); NNI 1, 2, 4 (128 x 128, 256 x 128, 256 x 256 tiles) -> 0, 1, 2
static constexpr int x3_slot(int OUT, int KW, int NNI) { return ((NNI >> 1) * 2 + OUT) * 2 + (KW == 3); }
typedef KernelTable<void (*)(ConvX3Args), 12> X3Table;
static X3Table x3_table() {
  X3Table t;
  for_values<1, 2, 4>([&](auto nni) { for_values<0, 1>([&](auto out) { for_values<1, 3>([&](auto kw) {
    t.put(x3_slot(out, kw, nni), conv1d_bf16x3_kernel<out, kw, nni>, ConvRings::LDS);
  }); }); });
  return t;
}

extern "C" int alvq_conv1d_bf16x3(const void* x, const void* wp, const float* bias, const void* skip1, const void* skip2,
                                  const void* mask, const void* post, void* y, void* y2, float* y_ncl, int B, int C, int M,
                                  int L, int KW, int relu, void* stream) {
  if (int rc = check_conv_args("alvq_conv1d_bf16x3", x, wp, skip1, skip2, mask, post, y, y2, y_ncl, B, C, M, L, KW, relu, nullptr,
                               nullptr))
    return rc;
  const long rows = alvq_nlc_rows(B, L);
  ConvX3Args a{{(const u16*)x, (const u16*)wp, bias, (const u16*)skip1, (const u16*)skip2, (const u16*)mask, (const u16*)post,
                (u16*)y, (u16*)y2, y_ncl, B, L, pad_to(C, 64), M, pad_to(M, 64), pad_to(M, WP_ROWS), relu ? 1 : 0,
                (int)(rows / ConvRings::R), pad_to(M, ConvRings::M) / ConvRings::M},
               nlc_plane_elems(B, L, C), (long)alvq_packed_weight_elems(M, C, KW), nlc_plane_elems(B, L, M)};
  static const X3Table table = x3_table();
  static DeviceOnce attr;
  if (attr.need()) table.raise_lds_limit();
  // 128-channel m-tile: outputs of at most 128 channels (no MFMA spent on padding channels), and problems whose 256 x 256
  // tiles would leave CUs idle (option "fx_narrow" = 0 switches it off here as in the f16mx kernel; "fx_rows" = 256 forces
  // the wide tile for the second case); results are bit-identical to the 256-wide tile's
  const int forced = (int)option(OPT_FX_ROWS);
  const bool narrow = option(OPT_FX_NARROW) != 0 && (M <= 128 || (forced != 256 && a.b.rtiles * a.b.mtiles < 192) || forced == 128);
  if (narrow) a.b.mtiles = pad_to(M, 128) / 128;
  // still fewer than ~3/4 of the CUs covered: 128-row tiles as well
  const bool small = narrow && forced != 256 && (a.b.rtiles * a.b.mtiles < 192 || forced == 128);
  if (small) a.b.rtiles = (int)(rows / 128);
  return table.launch(x3_slot(y ? 0 : 1, KW, small ? 1 : narrow ? 2 : 4), dim3(a.b.rtiles * a.b.mtiles), dim3(512),
                      (hipStream_t)stream, "alvq_conv1d_bf16x3", a);
}

extern "C" int64_t alvq_conv1d_wgrad_bf16x3_workspace_bytes(int B, int C, int M, int L, int KW) {
  return wgrad_workspace_bytes(B, C, M, L, KW, wgrad_x3_tile(KW), X3_BIAS_SPLITS);
}

extern "C" int alvq_conv1d_wgrad_bf16x3_splits(int B, int C, int M, int L, int KW, int nseg) {
  return wgrad_splits(B, C, M, L, KW, nseg, wgrad_x3_tile(KW));
}

// the weight gradient behind alvq_conv1d_wgrad_bf16x3 and its _multi form (no bias gradient there: dbias null)
static int wgrad_x3(const char* who, const void* const* dy, const void* const* x, int nseg, bool multi, float* dw, float* dbias,
                    void* workspace, int B, int C, int M, int L, int KW, int w_layout, int accumulate, hipStream_t s) {
  if (int rc = check_wgrad_args(who, dy, x, nseg, multi, dw, workspace, B, C, M, L, KW, w_layout, accumulate, false)) return rc;
  WgradX3Args a{};
  float* bpart;
  if (int rc = wgrad_plan("alvq_conv1d_wgrad_bf16x3", a, dy, x, nseg, workspace, B, C, M, L, KW, wgrad_x3_tile(KW), &bpart)) return rc;
  if (dbias) a.bias_partial = bpart;
  // conv1d_wgrad_bf16x3_kernel<KW, NCF> sits at [KW == 3]
  static const auto table = [] {
    KernelTable<void (*)(WgradX3Args), 2> t;
    for_values<1, 3>([&](auto kw) {
      constexpr int NCF = kw == 3 ? 2 : 4;
      t.put(kw == 3, conv1d_wgrad_bf16x3_kernel<kw, NCF>, wgrad_x3_lds<kw, NCF>());
    });
    return t;
  }();
  static DeviceOnce attr;
  if (attr.need()) table.raise_lds_limit();
  if (int rc = table.launch(KW == 3, dim3(a.mtiles * a.ctiles * a.splits), dim3(512), s, "alvq_conv1d_wgrad_bf16x3", a)) return rc;
  wgrad_reduce_launch((const float*)workspace, dw, a.splits, KW, M, C, w_layout, accumulate, s);
  if (dbias)     // single segment only (the shared residual weights have no bias)
    hipLaunchKernelGGL(wgrad_bias_reduce_kernel, dim3((M + 255) / 256), dim3(256), 0, s, (const float*)bpart, dbias, a.splits,
                       a.Mp, M, accumulate, (const float*)nullptr);
  return check_launch("alvq_conv1d_wgrad_bf16x3/reduce");
}

extern "C" int alvq_conv1d_wgrad_bf16x3(const void* dy, const void* x, float* dw, float* dbias, void* workspace, int B, int C,
                                        int M, int L, int KW, int w_layout, int accumulate, void* stream) {
  return wgrad_x3("alvq_conv1d_wgrad_bf16x3", &dy, &x, 1, false, dw, dbias, workspace, B, C, M, L, KW, w_layout, accumulate,
                  (hipStream_t)stream);
}

extern "C" int alvq_conv1d_wgrad_bf16x3_multi(const void* const* dy, const void* const* x, int nseg, float* dw, void* workspace,
                                              int B, int C, int M, int L, int KW, int w_layout, int accumulate, void* stream) {
  return wgrad_x3("alvq_conv1d_wgrad_bf16x3_multi", dy, x, nseg, true, dw, nullptr, workspace, B, C, M, L, KW, w_layout, accumulate,
                  (hipStream_t)stream);
}
