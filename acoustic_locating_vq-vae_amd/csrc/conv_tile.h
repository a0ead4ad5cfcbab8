// Device side of the forward / data-gradient convolution kernels (conv1d_bf16_kernel, conv1d_bf16_v2_kernel,
// conv1d_bf16_k3_kernel, conv1d_bf16x3_kernel, conv1d_f16mx_kernel): which tile a workgroup owns, where a 16-byte group lies
// in a slab of 64-byte LDS rows, the LDS-DMA primitives, the two rings of the two-plane kernels and the epilogues of the
// 16-bit kernels.  Device code only (host side: nlc_host.h).  Each kernel keeps its own MFMA schedule, waits and barriers;
// the weight-gradient kernels' counterpart is wgrad_tile.h, which takes its DMA primitives from here.
#pragma once
#include "alvq_common.h"
#include "bf16_common.h"

namespace alvq {

// ----------------------------------------------------------------------------------------------------------- tile origin
// Tile order: all m-tiles of a row tile are neighbours, and each XCD owns a contiguous run of tiles, so the workgroups
// resident on an XCD at one time share both operands through its L2 (W: one miss per m-tile per wave of workgroups;
// activation rows: one miss per row tile instead of one per m-tile).
struct ConvTileOrigin {
  int m0, r0;   // first output channel, first matrix row
};
template <int MT, int RT>
__device__ __forceinline__ ConvTileOrigin conv_tile_origin(const ConvBArgs& a) {
  const int tile = xcd_remap(blockIdx.x, a.mtiles * a.rtiles);
  return {(tile % a.mtiles) * MT, (tile / a.mtiles) * RT};
}

// ------------------------------------------------------------------------------------------- slabs of 64-byte LDS rows
// A slab row holds 32 channels = four 16-byte groups; group g of row r sits in slot g ^ key[quad], quad = (r >> 2) & 3,
// applied on the DMA SOURCE address (slab64_lane) and on the read address (slab64_frag16 / slab64_frag32), which makes
// every ds_read_b128 fragment read bank-conflict-free.  (The 128 x 128 kernel has 128-byte rows and its own row & 7 swizzle.)
//   SLAB_KEY_ROWS  {0,3,2,1}: weight slabs, and activation slabs read by the 32 x 32 lane pattern or per K-tile.
//   SLAB_KEY_TAPS  {0,2,0,2}: the width-3 bf16 kernel's activation slab.  The taps read it at row offsets 0, 1, 2, and
//     under {0,3,2,1} the shifted reads collide two-fold in two of every sixteen lanes of a ds_read_b128 bank group (18 %
//     of that kernel's LDS cycles were conflicts).  A 16-lane group takes four row quads with channel groups (a, b, b, a),
//     b = a ^ 1; rows shifted across a quad boundary keep their lane's group but take the next quad's key, so the key f
//     must make both {f0, f3, f1^1, f2^1} and {f0, f1, f2^1, f3^1} permutations of 0..3 -- (0, 2, 0, 2) does,
//     (0, 3, 2, 1) only the first.
enum SlabKey { SLAB_KEY_ROWS, SLAB_KEY_TAPS };
template <SlabKey KEY = SLAB_KEY_ROWS>
__device__ __forceinline__ int slab64_key(int quad) {
  return KEY == SLAB_KEY_TAPS ? (quad & 1) * 2 : (quad == 0 ? 0 : 4 - quad);
}

// Staging: a DMA piece is 16 rows x 64 B; lane i writes row i >> 2, slot i & 3 and must fetch the group that belongs there.
struct Slab64Lane {
  int row, grp;
};
template <SlabKey KEY = SLAB_KEY_ROWS>
__device__ __forceinline__ Slab64Lane slab64_lane(int lane) {
  const int key = slab64_key<KEY>((lane >> 4) & 3);
  return {lane >> 2, (lane & 3) ^ key};
}
// ... as ONE 32-bit byte offset into a [rows][Cp] matrix that serves every piece: the rest of a piece's source address is
// wave-uniform and goes into the DMA's SGPR base (these kernels have no room for hoisted 64-bit lane addresses)
template <SlabKey KEY = SLAB_KEY_ROWS>
__device__ __forceinline__ unsigned slab64_lane_off(int lane, int Cp) {
  const Slab64Lane s = slab64_lane<KEY>(lane);
  return (unsigned)(s.row * Cp + s.grp * 8) * 2u;
}

// Fragment reads: byte offset of 16-byte group g of block row r, read t rows further down (the tap).
// 16 x 16 MFMAs: lane (li = lane & 15, kq = lane >> 4) reads group kq of row li.
template <SlabKey KEY = SLAB_KEY_ROWS>
__device__ __forceinline__ int slab64_frag16(int li, int kq, int t) {
  const int r = li + t;
  return r * 64 + ((kq ^ slab64_key<KEY>((r >> 2) & 3)) << 4);
}
// 32 x 32 MFMAs: lane (r32 = lane & 31, g = lane >> 5) reads the groups g and 2 + g of row r32.
__device__ __forceinline__ int slab64_frag32(int r32, int g, int t) {
  const int r = r32 + t, key = slab64_key((r >> 2) & 3);
  return r * 64 + ((g ^ key) << 4);
}

// --------------------------------------------------------------------------------------------------------------- LDS-DMA
// 16 bytes per lane to LDS, 1 KB per wave-instruction.  The asm form (scalar base + one 32-bit lane offset, LDS address in
// M0) is invisible to the compiler, which would otherwise drain the whole ring (s_waitcnt vmcnt(0)) in front of every
// fragment read and hoist lane address + k * 16 rows into loop-invariant 64-bit VGPR pairs.
__device__ __forceinline__ void lds_dma16(const char* sbase, unsigned lds_dst, unsigned lane_off) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(lane_off), "s"(sbase), "s"(lds_dst)
               : "memory");
}
__device__ __forceinline__ unsigned lds_addr(const unsigned char* lds) {
  return (unsigned)(unsigned long)((const __attribute__((address_space(3))) unsigned char*)lds);
}
// The two primitives as a template parameter (WgradStager): 16 bytes per lane from base[elem] to lds + stage + off (stage,
// off: wave-uniform byte offsets, kept apart because the two forms add them differently -- the builtin to the pointer stage
// first, the asm form to the LDS address of `lds` itself, a constant; a sum formed the other way costs either kernel
// address-space checks inside its loop).
struct LdsDmaBuiltin {   // visible to the compiler, whose waits the v2 weight-gradient kernel counts against
  static __device__ __forceinline__ void copy(const u16* base, long elem, unsigned char* lds, int stage, int off) {
    unsigned char* const dst = lds + stage;
    glds16(base + elem, dst + off);
  }
};
struct LdsDmaAsm {
  static __device__ __forceinline__ void copy(const u16* base, long elem, unsigned char* lds, int stage, int off) {
    const unsigned dst = lds_addr(lds) + stage + off;
    lds_dma16((const char*)base, dst, (unsigned)(elem * 2));
  }
};

// ------------------------------------------------------------------------------------------ 256 x 256 tile, shared sizes
constexpr int V2_M = 256, V2_R = 256, V2_K = 32;
constexpr int V2_HALF = V2_M * V2_K * 2;          // 16384 B: one operand slab
constexpr int C_SLAB_STRIDE = V2_M + 4;           // fp32 C-slab row stride (floats)
constexpr int C_SLAB_BYTES = 64 * C_SLAB_STRIDE * 4;   // 66560 B of LDS used by the fp32-NCL store

// ------------------------------------------------------------------------------- the two rings of bf16x3 and f16mx
// A K-tile = (32 channels, one tap).  Two LDS-DMA rings of two stages each: the WEIGHT slabs of a K-tile (two planes, 32 KB)
// and the ACTIVATION slabs of a CHUNK of 32 channels (two planes; rows r0-PAD .. r0+255+PAD staged once, 34 KB) -- tap t
// reads the slab t rows further down, so a width-3 layer moves a third less through LDS-DMA.
struct ConvRings {
  static constexpr int M = 256, R = 256, K = 32;      // the largest tile; channels per K-tile
  static constexpr int SLAB = M * K * 2;              // 16384 B: one plane of a K-tile's weights
  static constexpr int WSTAGE = 2 * SLAB;
  static constexpr int XSLAB = 272 * 64;              // 272 rows x 64 B (258 used: 256 + a halo row either side)
  static constexpr int XSTAGE = 2 * XSLAB;
  static constexpr int XBASE = 2 * WSTAGE;            // first activation stage
  static constexpr int LDS = XBASE + 2 * XSTAGE;      // 135168 B
  static_assert(C_SLAB_BYTES <= LDS, "C slab must fit");
};

// Stages the rings of one workgroup (8 waves) whose tile is MT channels x RT rows: a wave owns 32 weight rows and 32
// activation rows of every plane (two 1-KB pieces each); of a narrow tile, waves 0 .. MT/32 - 1 stage the weights and
// waves 0 .. RT/32 - 1 the activations, the last of which adds the halo piece (slab rows RT, RT + 1) of a width-3 layer.
// plane 0 / 1: the hi / lo (H / Q) plane.  The sources are the KERNEL's locals, bound by reference as a lambda's captures are
// (copied into this object, the compiler merges the wave guards of neighbouring pieces, every kernel's register allocation
// moves and the width-3 f16mx kernels gain 32 bytes of scratch).  lane_off: slab64_lane_off, the one 32-bit VGPR; srow: the
// lane's row of a piece; wave-uniform, in bytes: wb, xb this wave's first weight row (m0 + 32 wave) and activation row
// (r0 - PAD + 32 wave) of the hi planes; tap_w, row16, wpl, xpl one tap of packed weights, 16 rows, hi -> lo plane.
// lds: the kernel's LDS array, handed over at each call (wgrad_tile.h says why).
template <int KW, int MT, int RT, bool PIECEWISE>
struct ConvRingStager {
  typedef ConvRings G;
  const int &wave, &srow;
  const unsigned& lane_off;
  const long &tap_w, &row16, &wpl, &xpl;
  const char *const &wb, *const &xb;
  __device__ __forceinline__ ConvRingStager(const int& wave_, const int& srow_, const unsigned& lane_off_, const long& tap_w_,
                                            const long& row16_, const long& wpl_, const long& xpl_, const char* const& wb_,
                                            const char* const& xb_)
      : wave(wave_), srow(srow_), lane_off(lane_off_), tap_w(tap_w_), row16(row16_), wpl(wpl_), xpl(xpl_), wb(wb_), xb(xb_) {}
  // piece k = 0..3 of K-tile t -> weight stage t & 1: (plane k >> 1, rows 16 (k & 1) ..)
  __device__ __forceinline__ void pieceW(unsigned char* lds, int t, int k) const { pieceW_<true>(lds, t, k); }
  // piece k = 0, 1 (+ 2: the halo rows) of one plane of a chunk's activation slab -> activation stage chunk & 1
  __device__ __forceinline__ void pieceX(unsigned char* lds, int chunk, int plane, int k) const { pieceX_<true>(lds, chunk, plane, k); }
  // Whole tiles.  PIECEWISE kernels (f16mx, which places single pieces between its MFMAs) check the wave rule per piece here
  // too, the others (bf16x3) once per tile -- the form each kernel had, and the one that keeps its registers.
  __device__ __forceinline__ void issueW(unsigned char* lds, int t) const {
    if constexpr (!PIECEWISE)
      if (wave * 32 >= MT) return;
    pieceW_<PIECEWISE>(lds, t, 0);
    pieceW_<PIECEWISE>(lds, t, 1);
    pieceW_<PIECEWISE>(lds, t, 2);
    pieceW_<PIECEWISE>(lds, t, 3);
  }
  __device__ __forceinline__ void issueX(unsigned char* lds, int chunk, int plane) const {
    if constexpr (!PIECEWISE)
      if (wave * 32 >= RT) return;
    pieceX_<PIECEWISE>(lds, chunk, plane, 0);
    pieceX_<PIECEWISE>(lds, chunk, plane, 1);
    pieceX_<PIECEWISE>(lds, chunk, plane, 2);
  }
  // chunk 0's activation slabs, K-tiles 0 and 1 (and, for width 1, chunk 1's slabs) staged and landed
  __device__ __forceinline__ void prologue(unsigned char* lds, int n, int nch) const {
    issueX(lds, 0, 0);
    issueX(lds, 0, 1);
    issueW(lds, 0);
    if (n > 1) issueW(lds, 1);
    if (KW == 1 && nch > 1) {
      issueX(lds, 1, 0);
      issueX(lds, 1, 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
 private:
  // GUARDED: the piece checks the narrow-tile wave rule itself (false only under a whole-tile issue that has checked it)
  template <bool GUARDED>
  __device__ __forceinline__ void pieceW_(unsigned char* lds, int t, int k) const {
    if constexpr (GUARDED)
      if (wave * 32 >= MT) return;
    const int chunk = t / KW, tap = t - chunk * KW;
    const unsigned dst = lds_addr(lds) + (t & 1) * G::WSTAGE + wave * 2048 + (k >> 1) * G::SLAB + (k & 1) * 1024;
    lds_dma16(wb + tap * tap_w + chunk * (G::K * 2) + (k >> 1) * wpl + (k & 1) * row16, dst, lane_off);
  }
  template <bool GUARDED>
  __device__ __forceinline__ void pieceX_(unsigned char* lds, int chunk, int plane, int k) const {
    const unsigned dst = lds_addr(lds) + G::XBASE + (chunk & 1) * G::XSTAGE + plane * G::XSLAB + wave * 2048;
    const char* xs = xb + plane * xpl + chunk * (G::K * 2);
    if constexpr (GUARDED)
      if (wave * 32 >= RT) return;
    if (k < 2) lds_dma16(xs + k * row16, dst + k * 1024, lane_off);
    else if (KW == 3 && wave == RT / 32 - 1 && srow < 2) lds_dma16(xs + 2 * row16, dst + 2048, lane_off);
  }
};

// -------------------------------------------------------------------------------------------------------- fp32-NCL store
// OUT == 1 (fp32 (B, M, L), bias only) of an MT x RT tile of 8 waves: RT / 64 slabs of 64 rows go through an fp32 LDS tile
// Cs[row][C_SLAB_STRIDE] so that lanes run along l.  write(Cs, slab): every wave that owns rows of the slab writes its
// fragments, D[i = m][j = row], as 16-byte groups of consecutive m.  Then lane = row (coalesced along l), loop over channels.
// SCALED: times *out_scale (null: 1; undoes a loss scale).  All waves must have finished reading the operand stages Cs
// overlays before the call.  (The 128 x 128 kernel keeps a store of its own: conv1d_bf16.hip says why.)
template <bool SCALED, int MT, int RT, class Write>
__device__ __forceinline__ void conv_store_ncl(const ConvBArgs& a, unsigned char* lds, int m0, int r0, int tid,
                                               const float* out_scale, Write write) {
  float oscale = 1.f;
  if constexpr (SCALED) oscale = out_scale ? *out_scale : 1.f;
  float* Cs = (float*)lds;
  for (int slab = 0; slab < RT / 64; ++slab) {
    write(Cs, slab);
    __syncthreads();
    const int Lp1 = a.L + 1, ndata = a.B * Lp1;
    const int rl = tid & 63, row = r0 + slab * 64 + rl;
    int b, l;
    if (row_valid(row, Lp1, ndata, &b, &l)) {
      for (int ml = tid >> 6; ml < MT; ml += 8) {
        const int m = m0 + ml;
        if (m >= a.M) break;
        const float v = Cs[rl * C_SLAB_STRIDE + ml] + (a.bias ? a.bias[m] : 0.f);
        a.y_ncl[((long)b * a.M + m) * a.L + l] = SCALED ? v * oscale : v;
      }
    }
    __syncthreads();   // the next slab overwrites Cs
  }
}

// 16 x 16 fragments of a wave, D[i = m][j = row], into Cs rows rl0 ..: lane (li, kq) holds 4 consecutive m = one 16-byte write
template <int CSTRIDE, int NMI, int NNI>
__device__ __forceinline__ void store_frags16(float* Cs, const f32x4 (&acc)[NMI][NNI], int li, int kq, int wm0, int rl0) {
#pragma unroll
  for (int mi = 0; mi < NMI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NNI; ++ni) {
      const int rl = rl0 + ni * 16 + li, ml = wm0 + mi * 16 + kq * 4;
      *(f32x4*)(Cs + rl * CSTRIDE + ml) = acc[mi][ni];
    }
}

// ------------------------------------------------------------------------------------- epilogues of the 16-bit kernels
struct FragSet {
  bf16x8_t a[8];
  bf16x8_t b[4];
};

// The register-direct bf16 / fp16 NLC epilogue of one wave's (NMI*16) m x (NNI*16) rows block of MFMA fragments:
// rows r0 + wn0 .., channels m0 + wm0 ..   (NMI even: fragments are swapped in pairs).  D[i = m][j = row], so lane (li, kq)
// of fragment (mi, ni) holds channels mi*16 + kq*4 .. +3 of row ni*16 + li.  v_permlane16_swap between the fragments mi and
// mi+1 first gives every lane 8 consecutive channels (lanes kq = 0, 2: channels (kq/2)*8.. of fragment mi; kq = 1, 3: of
// fragment mi+1), so loads and stores are 16 bytes per lane, the four lanes of a row cover 64 contiguous bytes and the next
// fragment pair completes the 128-byte line.  No LDS round trip, no barriers, and the skip / mask / post loads of different
// fragments are independent (they overlap instead of queueing behind one another).  The previous version transposed
// through LDS; its ~3000 VALU instructions per thread (software bf16 rounding, per-pass row decoding) made the epilogue
// 30 k cycles per tile -- 17 % of a width-3 tile's time, 37 % of a width-1 tile's.
template <int NMI, int NNI, int F16 = 0>
__device__ __forceinline__ void wave_epilogue_bf16(const ConvBArgs& a, const f32x4 (&acc)[NMI][NNI], int m0, int r0, int li,
                                                   int kq, int wm0, int wn0);

// The same for the operand sets of the data gradients, no load behind a store (below).
template <int NMI, int NNI, int F16, bool S1, bool S2, bool BITS>
__device__ __forceinline__ void wave_epilogue_dgrad16(const ConvBArgs& a, const f32x4 (&acc)[NMI][NNI], int m0, int r0, int li,
                                                      int kq, int wm0, int wn0);

// Epilogue of a 256 x 256 tile held as 8 x 4 MFMA fragments per wave (wave w: out-channels (w>>2)*128.., rows (w&3)*64..):
// OUT == 0 the register-direct one, OUT == 1 (rare at this tile size) four 64-row slabs through conv_store_ncl.
template <int OUT, int F16 = 0>
__device__ __forceinline__ void tile256_epilogue(const ConvBArgs& a, const f32x4 (&acc)[8][4], unsigned char* lds, int m0,
                                                 int r0, int wave, int tid, int li, int kq, int wm0) {
  if (OUT == 0) {
    // the data gradients' operand sets (a mask, as sign bits or as a tensor; + skip1; + skip1 + skip2) on a wave block that
    // lies inside Mop take the epilogue whose loads all go out in front of the stores; every other launch the general one
    const int wn0 = (wave & 3) * 64;
    const bool dgrad = (a.mask_bits || a.mask) && !a.bias && !a.y2 && !a.bits_out && !(a.relu & 1) && (a.skip1 || !a.skip2) &&
                       m0 + wm0 + 128 <= a.Mop;
    if (!dgrad) wave_epilogue_bf16<8, 4, F16>(a, acc, m0, r0, li, kq, wm0, wn0);
    else if (a.mask_bits) {
      if (a.skip2) wave_epilogue_dgrad16<8, 4, F16, true, true, true>(a, acc, m0, r0, li, kq, wm0, wn0);
      else if (a.skip1) wave_epilogue_dgrad16<8, 4, F16, true, false, true>(a, acc, m0, r0, li, kq, wm0, wn0);
      else wave_epilogue_dgrad16<8, 4, F16, false, false, true>(a, acc, m0, r0, li, kq, wm0, wn0);
    } else {
      if (a.skip2) wave_epilogue_dgrad16<8, 4, F16, true, true, false>(a, acc, m0, r0, li, kq, wm0, wn0);
      else if (a.skip1) wave_epilogue_dgrad16<8, 4, F16, true, false, false>(a, acc, m0, r0, li, kq, wm0, wn0);
      else wave_epilogue_dgrad16<8, 4, F16, false, false, false>(a, acc, m0, r0, li, kq, wm0, wn0);
    }
    return;
  }
  conv_store_ncl<true, V2_M, V2_R>(a, lds, m0, r0, tid, a.out_scale, [&](float* Cs, int slab) {
    if ((wave & 3) == slab) store_frags16<C_SLAB_STRIDE>(Cs, acc, li, kq, wm0, 0);
  });
}

// Written for few VALU instructions per value -- the epilogue of a 256 x 256 tile is 16 of these 8-channel groups per
// lane, and at ~100 instructions each it took twice the time its 2 bytes per element need on the way to HBM (measured by
// compiling it out: 13 us of a width-3 launch's 86 us per round, 10 of a width-1 launch's 41):
//  * a row block's pointers are formed once, the groups add constants to them;
//  * nothing is computed for operands that are absent (no bias -> no bias vector of zeros to add);
//  * gap / tail rows (one 16-row block in thirty holds one) are zeroed by a select on the four packed output words,
//    inside a wave-uniform branch, instead of a divergent branch around the whole group;
//  * the bias of a group that lies inside M is two 16-byte loads.
template <int NMI, int NNI, int F16>
__device__ __forceinline__ void wave_epilogue_bf16(const ConvBArgs& a, const f32x4 (&acc)[NMI][NNI], int m0, int r0, int li,
                                                   int kq, int wm0, int wn0) {
  static_assert(NMI % 2 == 0, "fragments are swapped in pairs");
  elem_saturate<F16>();
  unsigned watch = 0;
  const int Lp1 = a.L + 1, ndata = a.B * Lp1;
  const int mb0 = m0 + wm0 + (kq & 1) * 16 + (kq >> 1) * 8;      // this lane's 8 channels of fragment pair 0
#pragma unroll
  for (int ni = 0; ni < NNI; ++ni) {
    const int row = r0 + wn0 + ni * 16 + li;
    int b, l;
    const bool ok = row_valid(row, Lp1, ndata, &b, &l);
    const bool gaps = !__all(ok);
    const long o0 = (long)row * a.Mop + mb0;                      // element offset of the lane's first group
    // the skip / mask operands of the whole row block are requested before the first group is finished (a load ->
    // wait -> use chain per group is one L2 / HBM round trip each, sixteen per lane)
    u16x8 s1[NMI / 2], s2[NMI / 2], mk[NMI / 2];
#pragma unroll
    for (int mp = 0; mp < NMI; mp += 2) {
      if (m0 + wm0 + mp * 16 >= a.Mop) continue;
      if (a.skip1) s1[mp / 2] = *(const u16x8*)(a.skip1 + o0 + mp * 16);
      if (a.skip2) s2[mp / 2] = *(const u16x8*)(a.skip2 + o0 + mp * 16);
      if (a.mask && !a.mask_bits) mk[mp / 2] = *(const u16x8*)(a.mask + o0 + mp * 16);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mp = 0; mp < NMI; mp += 2) {
      if (m0 + wm0 + mp * 16 >= a.Mop) continue;        // Mop % 64 == 0 and the pair starts on a multiple of 32
      const long o = o0 + mp * 16;
      const int mb = mb0 + mp * 16;
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // odd rows (of 16 lanes) of the first operand <-> even rows of the second
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
        for (int e = 0; e < 8; ++e) v[e] += elem2f<F16>(s1[mp / 2][e]);
      }
      if (a.skip2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += elem2f<F16>(s2[mp / 2][e]);
      }
      if (a.relu & 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      if (a.mask_bits) {     // sign-extend bit e to a word and AND
        const int bt = (int)a.mask_bits[o >> 3];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __uint_as_float(__float_as_uint(v[e]) & (unsigned)((bt << (31 - e)) >> 31));
      } else if (a.mask) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (short)mk[mp / 2][e] > 0 ? v[e] : 0.f;   // a positive bf16 / fp16 is a positive int16
      }
      u32x4 out;
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = elem_pk<F16>(v[2 * e], v[2 * e + 1]);
      if (gaps) {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = ok ? out[e] : 0u;
      }
      *(u32x4*)(a.y + o) = out;
      if (F16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) fp16_watch(watch, out[e]);
      }
      if (a.y2) {
        const u16x8 ps = *(const u16x8*)(a.post + o);
        u32x4 out2;
#pragma unroll
        for (int e = 0; e < 4; ++e) out2[e] = elem_pk<F16>(v[2 * e] + elem2f<F16>(ps[2 * e]), v[2 * e + 1] + elem2f<F16>(ps[2 * e + 1]));
        if (gaps) {
#pragma unroll
          for (int e = 0; e < 4; ++e) out2[e] = ok ? out2[e] : 0u;
        }
        *(u32x4*)(a.y2 + o) = out2;
      }
      if (a.bits_out) {   // bit e = (stored y[e] > 0): a bf16 / fp16 in the upper half of a word is positive iff the word is, as an int
        unsigned bt = 0;
#pragma unroll
        for (int e = 7; e >= 0; --e) {
          const int half = (int)((e & 1) ? (out[e >> 1] & 0xffff0000u) : (out[e >> 1] << 16));
          const int t = half > 0 ? half : 0;
          bt = __builtin_amdgcn_alignbit(bt, 0u - (unsigned)t, 31);
        }
        a.bits_out[o >> 3] = (unsigned char)bt;
      }
    }
  }
  if (F16) fp16_report(watch, a.range_flag);
}

// wave_epilogue_bf16 for what the data gradients of a train step pass -- y = (acc [+ skip1 [+ skip2]]) under a mask (BITS: the
// sign bits of a 16-bit tensor; else a tensor, as the layers behind a bf16x3 forward pass it), no bias, ReLU, post or
// bits_out, every fragment pair inside Mop -- with the same values combined in the same order and stored
// to the same addresses, but NO wait on a load that was issued behind one of the wave's own stores.  gfx950 has one counter
// (vmcnt) for vector loads and stores and retires it in issue order, so waiting for such a load also waits for the store's
// write acknowledgement; the general epilogue reads its mask byte inside the group loop and requests every row block's skip
// operands behind the stores of the block before, which made a wave's sixteen groups sixteen store round trips in series,
// each as long as an acknowledgement takes when all 256 CUs drain a round together.  Which operands are present is a
// template argument here, not a branch: behind a branch the compiler cannot count the loads in flight and waits for all of
// them, stores included (s_waitcnt vmcnt(0)).  Requested before the first store: the lane's sixteen mask bytes and skip1 of
// all NNI row blocks (64 registers next to the 128 accumulators; the fragment registers are dead).  skip2, which only the
// stack's first layer passes, would be 64 more, and so would a mask tensor: they go one row block ahead -- block ni + 1's
// request is issued after block ni has been packed (16 registers) and before block ni's stores, so its wait leaves those
// stores outstanding.
template <int NMI, int NNI, int F16, bool S1, bool S2, bool BITS>
__device__ __forceinline__ void wave_epilogue_dgrad16(const ConvBArgs& a, const f32x4 (&acc)[NMI][NNI], int m0, int r0, int li,
                                                      int kq, int wm0, int wn0) {
  static_assert(NMI % 2 == 0, "fragments are swapped in pairs");
  constexpr int NP = NMI / 2;
  elem_saturate<F16>();
  unsigned watch = 0;
  const int Lp1 = a.L + 1, ndata = a.B * Lp1;
  const int mb0 = m0 + wm0 + (kq & 1) * 16 + (kq >> 1) * 8;      // this lane's 8 channels of fragment pair 0
  const long o00 = (long)(r0 + wn0 + li) * a.Mop + mb0;          // element offset of the lane's first group of row block 0
  const long oblk = (long)16 * a.Mop;                            // ... from one row block to the next
  int mbits[NNI][NP];
  u16x8 s1[NNI][NP], s2[NP], mk[NP];
  auto ahead = [&](int ni) {      // the operands that go one row block ahead
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (S2) s2[p] = *(const u16x8*)(a.skip2 + o00 + ni * oblk + p * 32);
      if (!BITS) mk[p] = *(const u16x8*)(a.mask + o00 + ni * oblk + p * 32);
    }
  };
  if (S1) {
#pragma unroll
    for (int ni = 0; ni < NNI; ++ni)
#pragma unroll
      for (int p = 0; p < NP; ++p) s1[ni][p] = *(const u16x8*)(a.skip1 + o00 + ni * oblk + p * 32);
  }
  ahead(0);
  // (the mask bytes last: were they the first thing every instantiation does, the compiler would merge them across the
  // caller's branch on the operand set and wait for them in front of it, one round trip before skip1 is even requested)
  if (BITS) {
#pragma unroll
    for (int ni = 0; ni < NNI; ++ni)
#pragma unroll
      for (int p = 0; p < NP; ++p) mbits[ni][p] = (int)a.mask_bits[(o00 + ni * oblk + p * 32) >> 3];
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int ni = 0; ni < NNI; ++ni) {
    int b, l;
    const bool ok = row_valid(r0 + wn0 + ni * 16 + li, Lp1, ndata, &b, &l);
    const bool gaps = !__all(ok);
    u32x4 out[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // odd rows (of 16 lanes) of the first operand <-> even rows of the second
        const u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][ni][e]), __float_as_uint(acc[2 * p + 1][ni][e]),
                                                         false, false);
        v[e] = __uint_as_float(r[0]);
        v[e + 4] = __uint_as_float(r[1]);
      }
      if (S1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += elem2f<F16>(s1[ni][p][e]);
      }
      if (S2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += elem2f<F16>(s2[p][e]);
      }
      if (BITS) {
        const int bt = mbits[ni][p];     // sign-extend bit e to a word and AND
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __uint_as_float(__float_as_uint(v[e]) & (unsigned)((bt << (31 - e)) >> 31));
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (short)mk[p][e] > 0 ? v[e] : 0.f;   // a positive bf16 / fp16 is a positive int16
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) out[p][e] = elem_pk<F16>(v[2 * e], v[2 * e + 1]);
      if (gaps) {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[p][e] = ok ? out[p][e] : 0u;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (ni + 1 < NNI) ahead(ni + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      *(u32x4*)(a.y + o00 + ni * oblk + p * 32) = out[p];
      if (F16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) fp16_watch(watch, out[p][e]);
      }
    }
  }
  if (F16) fp16_report(watch, a.range_flag);
}

}  // namespace alvq
