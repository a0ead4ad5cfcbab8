// Device side of the split-K weight-gradient kernels (conv1d_wgrad_bf16_v2_kernel, conv1d_wgrad_bf16_v3_kernel,
// conv1d_wgrad_bf16x3_kernel, conv1d_wgrad_f16mx_kernel): what a workgroup owns, how a K-tile is staged into LDS, where a
// lane's fragments lie in it and how the accumulators leave.  Device code only -- the host side of the same entry points is
// nlc_host.h.  Each kernel keeps its own MFMA schedule, ring depth and argument block; the pieces here take the argument
// block as a template parameter and use its fields by name (as wgrad_plan does on the host).
//
//   dW_t[m][c] = sum_rows dY[row][m] * X[row + t - pad][c]
//
// K-tile = 32 rows: per plane a dY slab [32][MT] and an X slab [32 + halo][CT], staged as 1-KB pieces (one
// global-load-to-LDS of a wave each).  LDS rows are whole 256-B bank lines, so the 32-B segment s of row r is stored at
// segment s ^ (r & 7) of its line: the swizzle is applied to the DMA's SOURCE address (wgrad_src_slot) and to the read
// address (wgrad_frag16_bases / wgrad_frag32_base).
#pragma once
#include "alvq_common.h"
#include "bf16_common.h"
#include "conv_tile.h"   // the DMA primitives LdsDmaBuiltin / LdsDmaAsm

namespace alvq {

// ------------------------------------------------------------------------------------------------------ workgroup decode
// split, (m, c) tile, first virtual row and K-tile count of this workgroup.  Rows are numbered through all segments:
// virtual row v = seg * total_rows + r (total_rows % 64 == 0, so neither a 64-row chunk nor a 32-row K-tile straddles two
// segments -- but a SPLIT may start in one segment and end in the next).
struct WgradWork {
  int split, m0, c0, rbeg;
  int n;   // K-tiles in this split (even; may be 0)
};
template <int MT, int CT, class Args>
__device__ __forceinline__ WgradWork wgrad_work(const Args& a) {
  const int ntile = a.mtiles * a.ctiles;
  const int id = xcd_remap(blockIdx.x, ntile * a.splits);
  const int split = id / ntile, t_id = id % ntile;
  const int rbeg = split * a.chunks_per_split * 64;
  const int rend = min(a.nseg * a.total_rows, rbeg + a.chunks_per_split * 64);
  return {split, (t_id / a.ctiles) * MT, (t_id % a.ctiles) * CT, rbeg, (rend - rbeg) / 32};
}

// 16-byte slot `slot` of LDS row `row` holds the logical slot (line, ((slot >> 1) & 7) ^ (row & 7), slot & 1)
__device__ __forceinline__ int wgrad_src_slot(int slot, int row) {
  return (slot & 16) | (((((slot >> 1) & 7) ^ (row & 7)) << 1) | (slot & 1));
}

// --------------------------------------------------------------------------------------------------------------- staging
// One stage of the LDS ring: plane by plane the dY slabs, then the X slabs.  (Host code sizes the ring from STAGE.)
template <int KW, int MT, int CT, int PLANES>
struct WgradSlabs {
  static_assert(PLANES == 1 || PLANES == 2, "one plane or a pair");
  static constexpr int PAD = (KW - 1) / 2;
  static constexpr int YRB = MT * 2, XRB = CT * 2;             // bytes per LDS row
  static constexpr int XROWS = KW == 1 ? 32 : 36;              // halo rows, rounded so the slab is whole 1-KB pieces
  static constexpr int YBYTES = 32 * YRB, XBYTES = XROWS * XRB;
  static constexpr int XOFF = PLANES * YBYTES;                 // first X slab of a stage
  static constexpr int STAGE = PLANES * (YBYTES + XBYTES);
  static constexpr int YPIECES = YBYTES / 1024, YROWS_PER_PIECE = 1024 / YRB;
  static constexpr int XPIECES = XBYTES / 1024, XROWS_PER_PIECE = 1024 / XRB;
  static constexpr int PER_WAVE = PLANES * (YPIECES / 8 + XPIECES / 8);   // DMAs per K-tile of a wave without the extra piece
  static_assert(YPIECES % 8 == 0, "the dY slab is whole pieces per wave");
};

// Stages K-tile after K-tile of one workgroup (8 waves) into the ring; piece p of a slab goes to wave p % 8.  The counted
// waits are built from the same constants as the issue loops, so a kernel cannot count differently from what it issues.
template <class Args, int KW, int MT, int CT, int PLANES, class Dma>
struct WgradStager {
  typedef WgradSlabs<KW, MT, CT, PLANES> S;

  const Args& a;
  const int wave, m0, c0;
  const int y_r, y_s, x_r, x_s;   // lane i of a piece covers bytes [16i, 16i + 16): row 16i / RB, 16-B slot (16i % RB) / 16
  int is_seg, is_row;             // segment and first row (inside it) of the K-tile the next issue() stages

  __device__ __forceinline__ WgradStager(const Args& a_, int wave_, int lane, const WgradWork& w)
      : a(a_), wave(wave_), m0(w.m0), c0(w.c0), y_r((lane * 16) / S::YRB), y_s(((lane * 16) % S::YRB) >> 4),
        x_r((lane * 16) / S::XRB), x_s(((lane * 16) % S::XRB) >> 4),
        is_seg(w.rbeg / a_.total_rows), is_row(w.rbeg - (w.rbeg / a_.total_rows) * a_.total_rows) {}

  // lds: the kernel's LDS array, handed over at each call (kept in this object, the pointer loses its address space across
  // the K loop and every copy pays a null check)
  __device__ __forceinline__ void issue(unsigned char* lds, int stage) {
    const int dst = stage * S::STAGE;
    // the second plane written out, not as a loop over pointer arrays: that form costs the f16mx kernel two more SGPRs
    const u16* const dy0 = a.dy[is_seg];
    const u16* dy1 = dy0;
    if constexpr (PLANES == 2) dy1 = a.dy[is_seg] + a.dy_plane;
    const u16* const x0 = a.x[is_seg];
    const u16* x1 = x0;
    if constexpr (PLANES == 2) x1 = a.x[is_seg] + a.x_plane;
    const int last_row = a.total_rows - 1;
#pragma unroll
    for (int q = 0; q < S::YPIECES / 8; ++q) {
      const int p = wave + 8 * q;
      const int lr = p * S::YROWS_PER_PIECE + y_r;
      const int mcol = min(m0 + wgrad_src_slot(y_s, lr) * 8, a.Mp - 8);   // tiles past Mp re-read the last chunk (discarded)
      const long elem = (long)(is_row + lr) * a.Mp + mcol;
      Dma::copy(dy0, elem, lds, dst, p * 1024);
      if constexpr (PLANES == 2) Dma::copy(dy1, elem, lds, dst, S::YBYTES + p * 1024);
    }
#pragma unroll
    for (int q = 0; q < (S::XPIECES + 7) / 8; ++q) {
      const int p = wave + 8 * q;
      if (p < S::XPIECES) {
        const int lr = p * S::XROWS_PER_PIECE + x_r;
        int gr = is_row - S::PAD + lr;                                         // halo rows outside the segment: its edge rows (zero)
        gr = gr < 0 ? 0 : (gr > last_row ? last_row : gr);
        const int ccol = min(c0 + wgrad_src_slot(x_s, lr) * 8, a.Cp - 8);
        const long elem = (long)gr * a.Cp + ccol;
        Dma::copy(x0, elem, lds, dst, S::XOFF + p * 1024);
        if constexpr (PLANES == 2) Dma::copy(x1, elem, lds, dst, S::XOFF + S::XBYTES + p * 1024);
      }
    }
    is_row += 32;
    if (is_row == a.total_rows) {   // the split goes on in the next segment
      is_row = 0;
      ++is_seg;
    }
  }

  // wait until all but the DMAs of the last `tiles` K-tiles (0..2) this wave issued have landed
  __device__ __forceinline__ void wait_keep(int tiles) const {
    const bool extra = (S::XPIECES % 8 != 0) && (wave < S::XPIECES % 8);   // this wave stages one more X piece (per plane)
    if (tiles == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (tiles == 1) {
      if (extra) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S::PER_WAVE + PLANES) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S::PER_WAVE) : "memory");
    } else {
      if (extra) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (S::PER_WAVE + PLANES)) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * S::PER_WAVE) : "memory");
    }
  }
};

// ------------------------------------------------------------------------------------------------------ transposing reads
// Two transposing reads (k rows r..r+3 and r+16..r+19 of one 16-column block, ROW_BYTES apart) -> one 8-element k fragment;
// through the builtin the two halves land directly in the halves of the fragment's register tuple (no copies).  The v2
// kernel reads through inline asm instead (tr_pair_issue in conv1d_wgrad_bf16_v2.hip says why).
template <class Frag>
__device__ __forceinline__ Frag wgrad_tr16_pair(const unsigned char* lds_row, int row_bytes) {
  typedef short s16x4_t __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) s16x4_t* lds_tr_ptr;
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(lds_row));
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(lds_row + 16 * row_bytes));
  return __builtin_bit_cast(Frag, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ----------------------------------------------------------------------------------------------------- fragment addresses
// 16 x 16 MFMAs (v2, bf16x3): a wave owns 64 m x (NCF * 16) c.  Lane (g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3)
// supplies the address of block row q, columns 4p..4p+3; block rows of group g: 4g + q (first read) and 16 + 4g + q (second
// read) -- the MFMA k index is permuted identically for both operands, which a contraction does not care about, so each
// half-wave reads 8 CONSECUTIVE rows: 8 distinct segments, conflict-free for every tap offset.
// Out: the lane's base offset inside a dY slab and, per tap, inside an X slab, and the column-block terms (wave-uniform:
// block index cb -> line = cb >> 3, segment = cb & 7).  m-fragment mi lies at ybase ^ yseg[mi], (tap t, c-fragment cf) at
// (xbase[t] ^ xseg[cf]) + xline[cf].  (Plain ints the kernel declares, here and below, not members of
// one object: held in a struct, the 32 x 32 bases moved the v3 kernel's register count.)
template <int KW, int NCF, int YRB, int XRB>
__device__ __forceinline__ void wgrad_frag16_bases(int lane, int wm0, int wc0, int& ybase, int (&xbase)[KW], int (&yseg)[4],
                                                   int (&xseg)[NCF], int (&xline)[NCF]) {
  const int krow = 4 * (lane >> 4) + ((lane >> 2) & 3), p4 = lane & 3;
  ybase = krow * YRB + ((krow & 7) << 5) + p4 * 8;
#pragma unroll
  for (int t = 0; t < KW; ++t) xbase[t] = (krow + t) * XRB + (((krow + t) & 7) << 5) + p4 * 8;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) yseg[mi] = ((wm0 >> 4) + mi) << 5;          // MT = 128 -> 8 blocks, one line
#pragma unroll
  for (int cf = 0; cf < NCF; ++cf) {
    const int cb = (wc0 >> 4) + cf;
    xseg[cf] = (cb & 7) << 5;
    xline[cf] = (cb >> 3) * 256;
  }
}

// 32 x 32 MFMAs (v3, the fp16 half of f16mx): lane l has i = l & 15 (lane of its 16-group), blk = (l >> 4) & 1 (which
// 16-column half of the 32-wide tile), g = l >> 5 (k group of the MFMA).  k-step s, group g covers the 8 rows 2q + g + 8s
// (first read) and 16 + 2q + g + 8s (second read), q = 0..3 -- rows of ONE parity per half-wave, which the (row & 7) swizzle
// spreads over 8 distinct segments (conv1d_wgrad_f16mx.hip has the long form).  The segment of fragment f of a wave is
// (wave part) + 2 f + (lane part) with the three parts in disjoint bits, so the XOR factors: offset = LANE BASE ^ (f << 6)
// -- one base register per operand and tap instead of one address register per fragment.
// The lane base of the slab with ROWB-byte rows whose wave part starts at column w0 (wm0 of dY, wc0 of X), for tap t (rows
// shifted by t; 0 for dY): tile f, k-step ks lie at (base ^ (f << 6)) + 8 ks ROWB.
// (i16, blk, g come from the kernel, which shares its g with the partial store: recomputed from the lane here and there, the
// compiler forms them differently and the kernels' register counts move.)
template <int ROWB>
__device__ __forceinline__ int wgrad_frag32_base(int i16, int blk, int g, int w0, int t) {
  const int row = 2 * (i16 >> 2) + g + t, p4 = i16 & 3;
  const int s = w0 >> 4;                             // first 16-column block (= 32-byte segment) of the wave
  return row * ROWB + p4 * 8 + (s >> 3) * 256 + ((((s & 7) ^ blk) ^ (row & 7)) << 5);
}

// ---------------------------------------------------------------------------------------------------------- partial store
// partial[split][t][m][c] = acc (fp32); D[i = m][j = c].  16 x 16: lane (li = lane & 15, kq = lane >> 4), register r holds
// m = 4 kq + r.  accb (do_bias): the products of the dY fragments with an all-ones operand -- every column j of D holds the
// same column sum of dY, lane li = 0 writes it to bias_partial[split][m].
template <int KW, int NCF, class Args>
__device__ __forceinline__ void wgrad_store16(const Args& a, const WgradWork& w, int lane, int wm0, int wc0,
                                              const f32x4 (&acc)[KW][4][NCF], bool do_bias, const f32x4 (&accb)[4]) {
  const int li = lane & 15, kq = lane >> 4;
  float* out = a.partial + (long)w.split * KW * a.M * a.C;
#pragma unroll
  for (int t = 0; t < KW; ++t)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int cf = 0; cf < NCF; ++cf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = w.m0 + wm0 + mi * 16 + kq * 4 + r;
          const int c = w.c0 + wc0 + cf * 16 + li;
          if (m < a.M && c < a.C) out[((long)t * a.M + m) * a.C + c] = acc[t][mi][cf][r];
        }
  if (do_bias && li == 0) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = w.m0 + wm0 + mi * 16 + kq * 4 + r;
        if (m < a.Mp) a.bias_partial[(long)w.split * a.Mp + m] = accb[mi][r];
      }
  }
}

// 32 x 32: lane (j = lane & 31, g = lane >> 5, the kernel's own), register q holds m = (q & 3) + 8 (q >> 2) + 4 g.
// SCALED: times `scale` (1 / loss scale, a power of two).
template <bool SCALED, int KW, int MF, int NC, class Args>
__device__ __forceinline__ void wgrad_store32(const Args& a, const WgradWork& w, int lane, int g, int wm0, int wc0,
                                              const f32x16 (&acc)[KW][MF][NC], float scale = 1.f) {
  const int jc = lane & 31;
  float* out = a.partial + (long)w.split * KW * a.M * a.C;
#pragma unroll
  for (int t = 0; t < KW; ++t)
#pragma unroll
    for (int mi = 0; mi < MF; ++mi)
#pragma unroll
      for (int cf = 0; cf < NC; ++cf)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int m = w.m0 + wm0 + mi * 32 + (q & 3) + 8 * (q >> 2) + 4 * g;
          const int c = w.c0 + wc0 + cf * 32 + jc;
          if (m < a.M && c < a.C) out[((long)t * a.M + m) * a.C + c] = SCALED ? acc[t][mi][cf][q] * scale : acc[t][mi][cf][q];
        }
}

}  // namespace alvq
