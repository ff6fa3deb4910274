// relayout_step.h -- the arithmetic of the read batch's relayout (reads_relayout.hip), free of HIP: plain C++17 that the device
// kernel and the host test driver (tests/c/relayout_step_driver.cc) compile alike.
//
// Source: a resident read batch (fastq_reads.hip) -- read r's sequence at src_start(r), a multiple of 64, zeros between reads.
// Destination: `count` reads at dst_start(i), ascending, dst_start(i) + len(i) <= dst_start(i + 1), every other byte of
// [0, total) the pad byte -- what layout_texts (scan_driver.hip) writes for the host list of the same sequences.  The two
// layouts search_many scans: the separator layout (a gap of pad bytes between reads: starts take every residue mod 16, a
// 64-byte block may hold several short reads) and the per-text layout (each read in whole blocks of its own; an empty read
// may take no block and share its start with the read behind it).  A lane makes one 64-byte block of the destination: its
// first read by binary search in the destination's starts, then every read that begins in front of the block's end, each
// read's share from the (in general unaligned) source with 16-byte loads and fastq_step.h's shift.
#pragma once
#include <cstddef>
#include <cstdint>

#include "fastq_step.h"
#include "hamming_step.h"

namespace sassy_hip {

// The bytes of word j (bytes 4j .. 4j + 3 of a block) that lie in the block's bytes [lo, hi), as a mask of whole bytes.
SASSY_FQ_HD uint32_t rl_word_mask(uint32_t j, uint32_t lo, uint32_t hi) {
  const uint32_t b0 = 4u * j;
  const uint32_t a = lo > b0 ? lo - b0 : 0u;
  const uint32_t e = hi > b0 ? (hi - b0 < 4u ? hi - b0 : 4u) : 0u;
  if (a >= e) return 0u;  // (so a < 4)
  const uint32_t upto = e >= 4u ? 0xFFFFFFFFu : (1u << (8u * e)) - 1u;
  const uint32_t below = (1u << (8u * a)) - 1u;
  return upto & ~below;
}

// The share of the read at [start, start + len) of the destination in the block that begins at pos: bytes [*lo, *hi) of the
// block; *off = where the block's byte 0 lies relative to the read's first byte (negative: the read begins inside the block).
// false: the read has no byte in the block.
SASSY_FQ_HD bool rl_segment(uint64_t pos, uint64_t start, uint64_t len, uint32_t* lo, uint32_t* hi, int64_t* off) {
  const uint64_t end = start + len, bend = pos + 64u;
  const uint64_t a = start > pos ? start : pos, e = end < bend ? end : bend;
  if (a >= e) return false;
  *lo = (uint32_t)(a - pos);
  *hi = (uint32_t)(e - pos);
  *off = (int64_t)pos - (int64_t)start;
  return true;
}

// Block b of the destination as sixteen little-endian words.  dst_start(i), len(i), src_start(i): read i of the `count` reads
// laid out; load16(a, w4): the 16 source bytes at offset a, a multiple of 16, into w4[0 .. 4) -- called only for a 16-byte
// piece that holds a byte of a read, which lies inside the source buffer because that begins and ends at a multiple of 16.
template <typename Load16, typename DstStart, typename Len, typename SrcStart>
SASSY_FQ_HD void rl_block(const Load16& load16, const DstStart& dst_start, const Len& len, const SrcStart& src_start, uint32_t count, uint64_t b,
                          uint8_t pad, uint32_t (&out)[16]) {
  const uint64_t pos = b * 64u;
  const uint32_t pad4 = 0x01010101u * pad;
#pragma unroll
  for (int j = 0; j < 16; ++j) out[j] = pad4;
  // the last read that starts at or in front of the block: every read in front of it ends where it starts, at the latest
  for (uint32_t t = ham_text_of(dst_start, count, pos); t < count && dst_start(t) < pos + 64u; ++t) {
    uint32_t lo, hi;
    int64_t off;
    if (!rl_segment(pos, dst_start(t), len(t), &lo, &hi, &off)) continue;
    const int64_t vsrc = (int64_t)src_start(t) + off;  // the source offset of the block's byte 0
    const int64_t a16 = vsrc & ~(int64_t)15;
    uint32_t w[20];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int64_t piece = a16 + 16 * j;
      w[4 * j] = w[4 * j + 1] = w[4 * j + 2] = w[4 * j + 3] = 0u;
      if (piece + 16 > vsrc + (int64_t)lo && piece < vsrc + (int64_t)hi) load16(piece, &w[4 * j]);
    }
    uint32_t seg[16];
    fq_shift_block(w, (uint32_t)(vsrc & 15), 64u, seg);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t m = rl_word_mask((uint32_t)j, lo, hi);
      out[j] = (out[j] & ~m) | (seg[j] & m);
    }
  }
}

// How many of a piece's 16 bytes at destination offset p lie in front of `total` (0 .. 16): 16 is one 16-byte store, less
// is the destination's last, short piece, stored byte by byte.
SASSY_FQ_HD uint32_t rl_piece_bytes(uint64_t p, uint64_t total) { return p >= total ? 0u : (total - p >= 16u ? 16u : (uint32_t)(total - p)); }

// Does one of the first `keep` (0 .. 4) bytes of w hold anything but A, C, G, T in either case?  (many_patterns.hip: acgt_only)
SASSY_FQ_HD bool rl_other_letter(uint32_t w, uint32_t keep) {
  bool bad = false;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t c = (w >> (8u * i)) & 0xDFu;
    if (i < keep && c != 'A' && c != 'C' && c != 'G' && c != 'T') bad = true;
  }
  return bad;
}

}  // namespace sassy_hip
