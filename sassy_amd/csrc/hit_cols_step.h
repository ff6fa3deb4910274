// hit_cols_step.h -- the column arithmetic of the grouped text pass's hit path (scan_kernel.hip: filter_dna_kernel<.., G = 2>)
// in 32-bit columns RELATIVE to the lane's origin, free of HIP: plain C++17 that the device kernel and the host test driver
// (tests/c/hit_cols_driver.cc) compile alike.
//
// A lane's origin is col_base = 64 * own_lo - 65536 (own_lo: the first block the lane owns), a multiple of 64 and negative
// for the first 1 024 blocks of a buffer.  Everything a lane computes about an occurrence lies within a few thousand columns
// of its own blocks, so the 64-bit forms (piece_end_cols, fuse_emit) spend their instructions on high halves that cancel.
// Here the absolute quantities come in once, as relative ones (HitBase), and every result is bit for bit the 64-bit form's:
// the driver holds that form and compares.
//
// DOMAIN: lane chunks whose relative columns fit 31 bits -- 65536 + 64 * (blocks per lane chunk) + kHitColsSlack < 2^31.
// hit_cols_fits says so, and the host refuses a geometry outside it where it chooses the blocks per lane (stream_geometry).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SASSY_HC_HD __host__ __device__ __forceinline__
#else
#define SASSY_HC_HD inline
#endif

namespace sassy_hip {

constexpr uint32_t kHitColsOrigin = 65536u;  // the relative column of the lane's first own column
constexpr uint32_t kHitColsSlack = 4096u;    // more than rem + k + 1 + a block, the furthest a mark lies behind its block
SASSY_HC_HD bool hit_cols_fits(uint64_t blocks_per_lane) { return blocks_per_lane < ((0x80000000ull - kHitColsOrigin - kHitColsSlack) >> 6); }

// What a lane knows about the buffer, relative to its origin (all per lane, computed once per segment).
struct HitBase {
  uint32_t max_rel;   // relative column of the buffer's last column (64 * n_blocks), at most 2^31 - 1 (then no clamp can hit)
  uint32_t zero_rel;  // relative column of absolute column 0, or 0 where that lies in front of relative column 0
  uint32_t base_blk;  // col_base / 64, its low 32 bits: the block of relative column 0
};
SASSY_HC_HD HitBase hit_base(int64_t col_base, int64_t max_col) {
  HitBase h;
  const int64_t top = max_col - col_base;
  h.max_rel = top < 0x7FFFFFFFll ? (uint32_t)(top > 0 ? top : 0) : 0x7FFFFFFFu;
  h.zero_rel = col_base < 0 ? (uint32_t)(-col_base) : 0u;
  h.base_blk = (uint32_t)(col_base >> 6);
  return h;
}
// relative column in front of block `it` of a lane whose iteration 0 is block blk0 and whose first own block is own_lo
// (blk0 <= own_lo <= blk0 + it: an evaluated block)
SASSY_HC_HD uint32_t hit_block_col(uint32_t blk0_minus_own_lo, uint32_t it) { return kHitColsOrigin + ((blk0_minus_own_lo + it) << 6); }

// 1-based index of the lowest / the highest set bit of hi:lo (!= 0) -- the 64-bit builtins: two v_ffbl / v_ffbh and a minimum on
// the device, no branch on the halves
SASSY_HC_HD uint32_t hc_ffs64(uint32_t lo, uint32_t hi) { return (uint32_t)__builtin_ctzll(((unsigned long long)hi << 32) | lo) + 1u; }
SASSY_HC_HD uint32_t hc_top64(uint32_t lo, uint32_t hi) { return 64u - (uint32_t)__builtin_clzll(((unsigned long long)hi << 32) | lo); }

struct HitCols {
  uint32_t lo, hi;
};
// A slot's two constants: with rem rows behind the piece and <= k edits (k <= kHitColsMaxK) the columns of an occurrence that
// ends at e are [e + rem - k, e + rem + k + 1] = [e - kHitColsMaxK + add_lo, e + add_hi], both adds >= 0 and below 256 for
// rem <= 246: a byte each.
constexpr uint32_t kHitColsMaxK = 7u;
SASSY_HC_HD uint32_t hit_add_lo(uint32_t rem, uint32_t k) { return rem + kHitColsMaxK - k; }
SASSY_HC_HD uint32_t hit_add_hi(uint32_t rem, uint32_t k) { return rem + k + 1u; }
// piece_end_cols: the end positions a match around the occurrences lo:hi (!= 0) of a piece can have -- with rem rows behind
// the piece and <= k edits, [e + rem - k, e + rem + k] for an occurrence that ends at e, + 1 column -- clamped to the
// buffer's columns 1 .. max.  bcol: hit_block_col of the block; add_lo / add_hi: the slot's (above).
SASSY_HC_HD HitCols hit_end_cols(uint32_t mask_lo, uint32_t mask_hi, uint32_t bcol, uint32_t add_lo, uint32_t add_hi, const HitBase& h) {
  const uint32_t c_lo = bcol - kHitColsMaxK + hc_ffs64(mask_lo, mask_hi) + add_lo;  // (>= 65536 - 6: never negative)
  const uint32_t c_hi = bcol + hc_top64(mask_lo, mask_hi) + add_hi;
  // absolute column 1 is relative column zero_rel + 1 where the origin is <= 0; behind it no clamp can hit: c_lo > 1 there
  const uint32_t min_rel = h.zero_rel + 1u;
  return HitCols{c_lo < min_rel ? min_rel : c_lo, c_hi > h.max_rel ? h.max_rel : c_hi};
}

struct HitWindow {
  uint32_t nv;     // whole 64-column blocks of the window, before the clamp at the buffer's beginning (the overflow test's)
  uint32_t first;  // queue entry .x: the window's first block
  uint32_t word;   // queue entry .y: skip << 14 | blocks << 6 | byte shift
};
// fuse_emit's arithmetic: the window of whole blocks that ends at relative column y and reports the end positions from x
// on, with `margin` + mk + 2 columns in front of x; it begins at byte 0 where the buffer begins inside it.
SASSY_HC_HD HitWindow hit_window(uint32_t x, uint32_t y, uint32_t margin, uint32_t mk, const HitBase& h) {
  HitWindow w;
  w.nv = (y - x + margin + mk + 2u + 63u) / 64u;
  uint32_t nv = w.nv;
  int32_t start = (int32_t)y - (int32_t)(64u * nv);
  if (start < (int32_t)h.zero_rel) {  // the buffer starts inside the window: whole blocks from byte 0
    start = (int32_t)h.zero_rel;
    nv = (y - h.zero_rel + 63u) / 64u;
  }
  const int32_t skip_s = (int32_t)x - 2 - start;
  const uint32_t skip = skip_s > 0 ? (uint32_t)skip_s : 0u;
  w.first = h.base_blk + ((uint32_t)start >> 6);
  w.word = (skip << 14) | (nv << 6) | ((uint32_t)start & 63u);
  return w;
}

}  // namespace sassy_hip
