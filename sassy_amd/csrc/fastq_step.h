// fastq_step.h -- the arithmetic of the FASTQ parse (fastq_reads.hip), free of HIP: plain C++17 that the device kernels and
// the host test driver (tests/c/fastq_step_driver.cc) compile alike.
//
// The definition is strict four-line FASTQ: split at '\n' (a final empty piece is no line), strip one trailing '\r' from each
// line; with L lines, record r is lines 4r .. 4r + 3: '@' id, sequence, '+' anything, quality.  Per byte p of an input of n bytes:
//   line start   p == 0 or byte p - 1 is '\n'; its line is the number of line starts in front of it, its class that number & 3
//   stripped     a '\r' whose next byte is '\n', or that is the input's last byte: the one '\r' its line loses
// A line's length is the next line's start (n + 1 where the input ends without a '\n', n where it ends with one) - 1 - its
// own start - 1 if it holds a stripped byte.  A lane works on 64 consecutive bytes as bit masks (bit b = byte b); from
// outside it needs one bit from either side -- "the byte in front is '\n' (or this is position 0)", "the byte behind is
// '\n' (or the input ends there)" -- and the number of line starts in front of it, which is a plain sum: counts are 32-bit
// inside a tile and a super-tile and 64-bit above.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SASSY_FQ_HD __host__ __device__ __forceinline__
#else
#define SASSY_FQ_HD inline
#endif

namespace sassy_hip {

constexpr uint32_t kFqLaneBytes = 64;
constexpr uint32_t kFqTileBytes = 4096;  // a wavefront's tile: 64 lanes x 64 bytes

SASSY_FQ_HD uint32_t fq_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(x);
#else
  return (uint32_t)__builtin_popcountll(x);
#endif
}
// the bits below bit i, 0 <= i <= 64
SASSY_FQ_HD uint64_t fq_below(uint32_t i) { return i >= 64 ? ~0ull : (1ull << i) - 1ull; }

// bit b of the result: byte b of v equals the byte that c4 repeats four times
SASSY_FQ_HD uint32_t fq_eq_bits4(uint32_t v, uint32_t c4) {
  const uint32_t z = v ^ c4;
  const uint32_t t = ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;  // bit 7 of every zero byte of z, exactly
  return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}
// the same over a lane's 64 bytes as sixteen little-endian words
SASSY_FQ_HD uint64_t fq_eq_bits64(const uint32_t (&w)[16], uint8_t c) {
  const uint32_t c4 = 0x01010101u * c;
  uint64_t m = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) m |= (uint64_t)fq_eq_bits4(w[j], c4) << (4 * j);
  return m;
}

// The masks of one lane.  nl, cr: byte b is '\n', '\r'; len: how many of the 64 bytes lie inside the input (the masks hold no
// bit at len or above); prev_nl: the byte in front of the lane is '\n', or the lane begins the input; next_end: the byte
// behind the lane's 64 is '\n' or lies behind the input (read only when len == 64).
struct FastqLane {
  uint64_t ls;     // line starts
  uint64_t strip;  // stripped '\r'
};
SASSY_FQ_HD FastqLane fq_lane(uint64_t nl, uint64_t cr, uint32_t len, bool prev_nl, bool next_end) {
  const uint64_t valid = fq_below(len);
  FastqLane L;
  L.ls = ((nl << 1) | (prev_nl ? 1ull : 0ull)) & valid;
  // bit b: byte b + 1 is '\n' or the input ends behind byte b
  uint64_t after = nl >> 1;
  if (len == 64) after |= next_end ? 1ull << 63 : 0ull;
  else if (len > 0) after |= 1ull << (len - 1);
  L.strip = valid & cr & after;
  return L;
}

// A lane's share in the scan: its line starts.  `front`: the line starts in front of the lane.
SASSY_FQ_HD uint32_t fq_count(const FastqLane& L) { return fq_popc(L.ls); }
// the line that starts at bit i of the lane (a bit of L.ls), and its class
SASSY_FQ_HD uint64_t fq_line_of_start(const FastqLane& L, uint64_t front, uint32_t i) { return front + fq_popc(L.ls & fq_below(i)); }
SASSY_FQ_HD uint32_t fq_class(uint64_t line) { return (uint32_t)(line & 3ull); }
// the line that holds byte i of the lane: the last line start at or in front of it (position 0 is one, so there is one)
SASSY_FQ_HD uint64_t fq_line_of_byte(const FastqLane& L, uint64_t front, uint32_t i) { return front + fq_popc(L.ls & fq_below(i + 1)) - 1ull; }

// The two-level scan's summaries are counts of line starts: a tile's and a super-tile's fit 32 bits (at most one per byte),
// the sums over super-tiles are 64-bit.  What lies in front of a tile is what lies in front of its super-tile plus the
// tiles in front of it inside the super-tile.
SASSY_FQ_HD uint64_t fq_front(uint64_t super_front, uint32_t tile_front) { return super_front + tile_front; }

// Where the line behind the input's last one would start: the `next start` of the last line.
SASSY_FQ_HD uint64_t fq_virtual_start(uint64_t n, bool last_is_nl) { return last_is_nl ? n : n + 1; }
// A line's length from its start, the next line's start and whether it holds a stripped '\r'.
SASSY_FQ_HD uint64_t fq_line_len(uint64_t start, uint64_t next_start, bool stripped) { return next_start - 1 - start - (stripped ? 1ull : 0ull); }

// What breaks the four-line shape first, given L lines and the smallest line of class 0 without '@' or of class 2 without
// '+' (bad_line, UINT64_MAX: none): the smallest malformed record and the rule it breaks.
enum FastqRule : uint32_t { kFqOk = 0, kFqNoAt = 1, kFqShort = 2, kFqNoPlus = 3 };
struct FastqVerdict {
  uint64_t record;
  FastqRule rule;
};
SASSY_FQ_HD FastqVerdict fq_verdict(uint64_t n_lines, uint64_t bad_line) {
  const uint64_t none = ~0ull;
  const uint64_t cut = (n_lines & 3ull) ? n_lines >> 2 : none;  // the record the input ends inside
  const uint64_t marked = bad_line == none ? none : bad_line >> 2;
  if (cut == none && marked == none) return FastqVerdict{0, kFqOk};
  if (marked <= cut) {
    // (the same record: a missing '@' comes first, then the missing lines, then a missing '+')
    if (marked < cut || (bad_line & 3ull) == 0) return FastqVerdict{marked, (bad_line & 3ull) == 0 ? kFqNoAt : kFqNoPlus};
  }
  return FastqVerdict{cut, kFqShort};
}

// The layout rule: a sequence starts at a multiple of 64, seq_start is the exclusive scan of the lengths rounded up to 64.
// An empty sequence takes no block and shares its start with the read behind it; trailing empty reads start at the total.
SASSY_FQ_HD uint64_t fq_round64(uint64_t x) { return (x + 63ull) & ~63ull; }
// `count` lengths into starts; returns the layout's bytes
inline uint64_t fq_layout(const uint64_t* lens, uint64_t count, uint64_t* starts) {
  uint64_t at = 0;
  for (uint64_t r = 0; r < count; ++r) {
    starts[r] = at;
    at += fq_round64(lens[r]);
  }
  return at;
}

// One 64-byte block of the layout from an unaligned source: src16[0 .. 20) are the twenty words from the source address
// rounded down to 16, shift = source address & 15, keep = bytes of the block that belong to the read (0 .. 64); out[j] is
// word j of the block, zero behind `keep`.
SASSY_FQ_HD void fq_shift_block(const uint32_t (&src16)[20], uint32_t shift, uint32_t keep, uint32_t (&out)[16]) {
  uint32_t w[20];
#pragma unroll
  for (int j = 0; j < 20; ++j) w[j] = src16[j];
  if (shift & 8u) {
#pragma unroll
    for (int j = 0; j < 18; ++j) w[j] = w[j + 2];
  }
  if (shift & 4u) {
#pragma unroll
    for (int j = 0; j < 17; ++j) w[j] = w[j + 1];
  }
  const uint32_t sh = 8u * (shift & 3u);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint64_t two = ((uint64_t)w[j + 1] << 32) | w[j];
    const uint32_t v = (uint32_t)(two >> sh);
    const uint32_t left = keep > 4u * j ? keep - 4u * j : 0u;  // bytes of this word that are kept
    out[j] = left >= 4u ? v : (v & ((1u << (8u * left)) - 1u));
  }
}

}  // namespace sassy_hip
