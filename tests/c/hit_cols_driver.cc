// tests/c/hit_cols_driver.cc -- the 32-bit relative column arithmetic of the grouped pass's hit path
// (sassy_amd/csrc/hit_cols_step.h) against the 64-bit forms it replaces in the kernel (scan_kernel.hip: piece_end_cols,
// fuse_emit), which are restated here as the reference.  A stand-alone program: its own main, no HIP.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o hit_cols_driver hit_cols_driver.cc
//   ./hit_cols_driver      prints "ok cols=.. clamped_lo=.. clamped_hi=.. windows=.. from_zero=.. negative_base=.. high_base=.." or the first mismatch
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../sassy_amd/csrc/hit_cols_step.h"

using namespace sassy_hip;

namespace {

struct U2 {
  uint32_t x, y;
};

// ---- the reference: the kernel's 64-bit forms
U2 ref_piece_end_cols(uint64_t bits, uint64_t b, int64_t rem, int64_t k, int64_t max_col, int64_t col_base) {
  const int64_t e_lo = (int64_t)(b * 64) + (__builtin_ctzll(bits) + 1);   // first end position
  const int64_t e_hi = (int64_t)(b * 64) + 64 - __builtin_clzll(bits);    // last end position
  int64_t c_lo = e_lo + rem - k, c_hi = e_hi + rem + k + 1;
  if (c_lo < 1) c_lo = 1;
  if (c_hi > max_col) c_hi = max_col;
  return U2{(uint32_t)(c_lo - col_base), (uint32_t)(c_hi - col_base)};
}
struct RefWindow {
  uint32_t nv0, first, word;
};
RefWindow ref_fuse_emit(uint32_t x, uint32_t y, uint32_t margin, uint32_t mk, int64_t col_base) {
  uint32_t nv = (y - x + margin + mk + 2u + 63u) / 64u;
  const uint32_t nv0 = nv;
  const int64_t end = col_base + (int64_t)y;
  int64_t start = end - 64 * (int64_t)nv;
  if (start < 0) {
    start = 0;
    nv = (uint32_t)((end + 63) / 64);
  }
  const int64_t skip64 = (col_base + (int64_t)x - 2) - start;
  const uint32_t skip = skip64 > 0 ? (uint32_t)skip64 : 0u;
  return RefWindow{nv0, (uint32_t)(start >> 6), (skip << 14) | (nv << 6) | (uint32_t)(start & 63)};
}

struct Counts {
  long cols = 0, clamped_lo = 0, clamped_hi = 0, windows = 0, from_zero = 0, negative_base = 0, high_base = 0;
};

constexpr uint32_t kMargin = 64, kMergeGap = 32;

// one lane: own_lo its first block, n_blocks the buffer's, blocks own_lo .. own_lo + span - 1 evaluated (iteration 0 is
// block own_lo - back, or 0)
bool lane(uint64_t own_lo, uint64_t n_blocks, uint32_t span, uint32_t back, const uint64_t* masks, int n_masks, Counts* n) {
  const int64_t col_base = (int64_t)(own_lo * 64) - 65536;
  const int64_t max_col = (int64_t)(n_blocks * 64);
  const uint64_t blk0 = own_lo > back ? own_lo - back : 0;
  const HitBase h = hit_base(col_base, max_col);
  const uint32_t ev_lo = (uint32_t)(own_lo - blk0);
  if (col_base < 0) ++n->negative_base;
  if (own_lo >> 31) ++n->high_base;
  for (uint32_t it = ev_lo; it < ev_lo + span && blk0 + it < n_blocks; ++it) {
    const uint64_t b = blk0 + it;
    const uint32_t bcol = hit_block_col(0u - ev_lo, it);
    if ((int64_t)bcol != (int64_t)(b * 64) - col_base) { printf("bcol: own_lo %llu it %u\n", (unsigned long long)own_lo, it); return false; }
    for (int mi = 0; mi < n_masks; ++mi) {
      const uint64_t bits = masks[mi];
      for (uint32_t rem = 0; rem <= 120; rem += (mi < 64 ? 1 : 7)) {
        for (uint32_t k = 0; k <= 7; ++k) {
          const U2 want = ref_piece_end_cols(bits, b, (int64_t)rem, (int64_t)k, max_col, col_base);
          const HitCols got = hit_end_cols((uint32_t)bits, (uint32_t)(bits >> 32), bcol, hit_add_lo(rem, k), hit_add_hi(rem, k), h);
          if (hit_add_lo(rem, k) > 255u || hit_add_hi(rem, k) > 255u) { printf("a slot's adds are bytes\n"); return false; }
          if (got.lo != want.x || got.hi != want.y) {
            printf("cols: own_lo %llu n_blocks %llu b %llu bits %016llx rem %u k %u: got %u %u want %u %u\n", (unsigned long long)own_lo,
                   (unsigned long long)n_blocks, (unsigned long long)b, (unsigned long long)bits, rem, k, got.lo, got.hi, want.x, want.y);
            return false;
          }
          ++n->cols;
          const int64_t raw_lo = (int64_t)(b * 64) + __builtin_ctzll(bits) + 1 + rem - k;
          const int64_t raw_hi = (int64_t)(b * 64) + 64 - __builtin_clzll(bits) + rem + k + 1;
          if (raw_lo < 1) ++n->clamped_lo;
          if (raw_hi > max_col) ++n->clamped_hi;
          if (want.x > want.y || (mi >= 64 && (rem + k) % 5)) continue;
          // the windows fuse_add_range can ask for around these columns: the run as it is, with and without the margin,
          // grown by a merge gap, and the first part of a split run
          const uint32_t mks[3] = {k + 8u, rem + 12u + k, 128u + k};
          const uint32_t ys[3] = {want.y, want.y + kMergeGap, want.x + 64u * 8u - 1u};
          for (uint32_t mk : mks)
            for (uint32_t y : ys)
              for (uint32_t margin : {0u, kMargin}) {
                const RefWindow ww = ref_fuse_emit(want.x, y, margin, mk, col_base);
                const HitWindow gw = hit_window(want.x, y, margin, mk, h);
                if (gw.nv != ww.nv0 || gw.first != ww.first || gw.word != ww.word) {
                  printf("window: own_lo %llu x %u y %u margin %u mk %u: got %u %08x %08x want %u %08x %08x\n", (unsigned long long)own_lo, want.x, y,
                         margin, mk, gw.nv, gw.first, gw.word, ww.nv0, ww.first, ww.word);
                  return false;
                }
                ++n->windows;
                if (col_base + (int64_t)y - 64 * (int64_t)ww.nv0 < 0) ++n->from_zero;
              }
        }
      }
    }
  }
  return true;
}

}  // namespace

int main() {
  // every single bit, and pairs of bits, of a 64-column mask
  static uint64_t masks[64 + 64 * 63 / 2];
  int n_masks = 0;
  for (int i = 0; i < 64; ++i) masks[n_masks++] = 1ull << i;
  for (int i = 0; i < 64; ++i)
    for (int j = i + 1; j < 64; ++j) masks[n_masks++] = (1ull << i) | (1ull << j);
  Counts n;
  if (!hit_cols_fits(8) || !hit_cols_fits(1u << 20) || hit_cols_fits(1ull << 25) || hit_cols_fits(0x7FFFFFFFull)) { printf("hit_cols_fits\n"); return 1; }
  const uint32_t bpl = 8;
  // the buffer's first columns (the clamp to 1, windows that begin before byte 0): own_lo 0, 1, 2, with both warm-ups
  for (uint64_t own_lo : {0ull, 1ull, 2ull, 3ull})
    for (uint32_t back : {1u, 2u})
      if (!lane(own_lo, 4096, 3, back, masks, n_masks, &n)) return 1;
  // own_lo below 1 024 blocks: col_base is negative, byte 0 lies at a positive relative column
  for (uint64_t own_lo : {8ull, 512ull, 1016ull, 1023ull, 1024ull, 1025ull})
    if (!lane(own_lo, 1u << 20, 2, 1, masks, 64, &n)) return 1;
  // the buffer's last columns (the clamp to max_col): lanes that own the last blocks, of small and of huge buffers
  for (uint64_t n_blocks : {3000ull, (1ull << 31) + 77ull, (1ull << 32) - 5ull})
    for (uint64_t d : {1ull, 2ull, 3ull})
      if (!lane(n_blocks - d, n_blocks, 3, 1 + (uint32_t)(d & 1), masks, d == 1 ? n_masks : 64, &n)) return 1;
  // own_lo just under 2^32 - bpl, and a buffer that goes on behind it
  for (uint64_t own_lo : {(1ull << 32) - bpl - 1, (1ull << 32) - 2 * bpl, (1ull << 31) - 1, 1ull << 31})
    if (!lane(own_lo, (1ull << 32) - 1, 2, 2, masks, 64, &n)) return 1;
  // a lane chunk at the end of the domain: its last block's columns still fit 31 bits
  {
    const uint64_t far = ((0x80000000ull - kHitColsOrigin - kHitColsSlack) >> 6) - 2;
    if (!hit_cols_fits(far + 1)) { printf("domain\n"); return 1; }
    const uint64_t own_lo = 5000;
    const int64_t col_base = (int64_t)(own_lo * 64) - 65536;
    const HitBase h = hit_base(col_base, (int64_t)1 << 40);
    const uint64_t b = own_lo + far;
    const uint32_t bcol = hit_block_col(0u - 1u, 1u + (uint32_t)far);
    for (int i = 0; i < 64; ++i) {
      const U2 want = ref_piece_end_cols(masks[i], b, 120, 7, (int64_t)1 << 40, col_base);
      const HitCols got = hit_end_cols((uint32_t)masks[i], (uint32_t)(masks[i] >> 32), bcol, hit_add_lo(120, 7), hit_add_hi(120, 7), h);
      if (got.lo != want.x || got.hi != want.y || (got.hi >> 31)) { printf("far block: bit %d\n", i); return 1; }
      ++n.cols;
    }
  }
  printf("ok cols=%ld clamped_lo=%ld clamped_hi=%ld windows=%ld from_zero=%ld negative_base=%ld high_base=%ld\n", n.cols, n.clamped_lo, n.clamped_hi,
         n.windows, n.from_zero, n.negative_base, n.high_base);
  return 0;
}
