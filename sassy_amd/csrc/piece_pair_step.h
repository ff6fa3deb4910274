// piece_pair_step.h -- the piece test of the grouped text pass (scan_kernel.hip: filter_dna_kernel<.., G = 2>) on a PAIR of
// 64-byte blocks, free of HIP: plain C++17 that the device kernel and the host test driver (tests/c/piece_pair_driver.cc)
// compile alike.
//
// A block's text comes as two code planes of 64 bits (bit c of plane p = bit p of the 2-bit code of text byte c), a piece
// as two row masks (bit j = bit p of row j's code) -- the kernel holds their complements, ~P0 / ~P1.  Slot s has an
// occurrence that ENDS at column c iff for every row j the text's code at column c - (Q - 1 - j) is the row's: row j sits
// d = Q - 1 - j columns left of the detection column.  Per distance d the planes are shifted by d columns (the 32 columns
// in front of a block come from the previous block's high halves) and every slot's accumulator takes
//     acc &= plane0_shifted ^ n0,  acc &= plane1_shifted ^ n1        n = ~0 where the row's bit is 0, else 0
// -- one v_bitop3_b32 each per plane and 32-column half.
//
// The constants n are wave-uniform.  As scalar operands they halve the rate of every vector instruction that reads them
// (profiles/r12_piece_pair.txt section 1: 4.5 against 2.8 cycles), so the pair step reads them into VECTOR registers, from a
// table [row][slot]{n0, n1} the workgroup writes once (device: LDS, one broadcast 16-byte read per row and two slots), and
// uses each for the four words of both blocks: eight accumulator updates per pair of reads instead of four per pair of
// scalar extracts.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SASSY_PP_HD __host__ __device__ __forceinline__
#else
#define SASSY_PP_HD inline
#endif

namespace sassy_hip {

// a & (b ^ c)
SASSY_PP_HD uint32_t pp_and_xor(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x60);
#else
  return a & (b ^ c);
#endif
}
// the word `hi` with its columns moved up by d, the top d columns of `lo` (the 32 columns in front) coming in below; 0 <= d < 32
SASSY_PP_HD uint32_t pp_shift_in(uint32_t hi, uint32_t lo, int d) {
  if (d == 0) return hi;
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, 32 - d);
#else
  return (hi << d) | (lo >> (32 - d));
#endif
}
// ~0 where bit j of `bits` is set, else 0
SASSY_PP_HD uint32_t pp_row_word(uint32_t bits, int j) { return (uint32_t)-(int32_t)((bits >> j) & 1u); }

// a block's two code planes, in the order the plane store keeps them
struct PiecePlanes {
  uint32_t p0l, p0h, p1l, p1h;  // plane 0 columns 0 .. 31, 32 .. 63; plane 1 likewise
};
// the table's entry of one row and two neighbouring slots
struct alignas(16) PieceRow4 {
  uint32_t n0a, n1a, n0b, n1b;
};

// dwords of the table of a Q-row piece test with NS slots
template <int Q, int NS>
constexpr uint32_t piece_row_table_words() { return (uint32_t)(Q * NS * 2); }
// Entries first, first + stride, ... of the table (one entry = one row of one slot; Q * NS entries) from the slots' ~P0 /
// ~P1 row masks: nb(slot, plane).  A workgroup fills it with first = the thread, stride = its size; a host caller with 0, 1.
template <int Q, int NS, typename Masks>
SASSY_PP_HD void piece_row_table_fill(uint32_t* tab, uint32_t first, uint32_t stride, const Masks& nb) {
  for (uint32_t e = first; e < (uint32_t)(Q * NS); e += stride) {
    const uint32_t j = e / (uint32_t)NS, s = e % (uint32_t)NS;
    tab[2 * e] = pp_row_word(nb(s, 0), (int)j);
    tab[2 * e + 1] = pp_row_word(nb(s, 1), (int)j);
  }
}

// The pair step.  a, b: the planes of two consecutive blocks; prev0 / prev1: the high halves of the planes of the block in
// front of a -- on return b's, for the pair behind; tab: the table above (16-byte aligned).  al / ah (bl / bh): per slot
// the occurrence mask of a's (b's) columns 0 .. 31 / 32 .. 63.
template <int Q, int NS>
SASSY_PP_HD void piece_pair_step(const PiecePlanes& a, const PiecePlanes& b, uint32_t& prev0, uint32_t& prev1, const uint32_t* tab,
                                 uint32_t (&al)[NS], uint32_t (&ah)[NS], uint32_t (&bl)[NS], uint32_t (&bh)[NS]) {
  static_assert(Q >= 1 && Q <= 32 && NS % 2 == 0, "rows reach at most one half back; the table is read two slots at a time");
#pragma unroll
  for (int s = 0; s < NS; ++s) al[s] = ah[s] = bl[s] = bh[s] = 0xFFFFFFFFu;
#pragma unroll
  for (int d = 0; d < Q; ++d) {
    const int j = Q - 1 - d;
    const uint32_t a0l = pp_shift_in(a.p0l, prev0, d), a0h = pp_shift_in(a.p0h, a.p0l, d);
    const uint32_t b0l = pp_shift_in(b.p0l, a.p0h, d), b0h = pp_shift_in(b.p0h, b.p0l, d);
    const uint32_t a1l = pp_shift_in(a.p1l, prev1, d), a1h = pp_shift_in(a.p1h, a.p1l, d);
    const uint32_t b1l = pp_shift_in(b.p1l, a.p1h, d), b1h = pp_shift_in(b.p1h, b.p1l, d);
#pragma unroll
    for (int s = 0; s < NS; s += 2) {
      const PieceRow4 c = *reinterpret_cast<const PieceRow4*>(tab + (size_t)(j * NS + s) * 2);
      al[s] = pp_and_xor(al[s], a0l, c.n0a);
      ah[s] = pp_and_xor(ah[s], a0h, c.n0a);
      bl[s] = pp_and_xor(bl[s], b0l, c.n0a);
      bh[s] = pp_and_xor(bh[s], b0h, c.n0a);
      al[s] = pp_and_xor(al[s], a1l, c.n1a);
      ah[s] = pp_and_xor(ah[s], a1h, c.n1a);
      bl[s] = pp_and_xor(bl[s], b1l, c.n1a);
      bh[s] = pp_and_xor(bh[s], b1h, c.n1a);
      al[s + 1] = pp_and_xor(al[s + 1], a0l, c.n0b);
      ah[s + 1] = pp_and_xor(ah[s + 1], a0h, c.n0b);
      bl[s + 1] = pp_and_xor(bl[s + 1], b0l, c.n0b);
      bh[s + 1] = pp_and_xor(bh[s + 1], b0h, c.n0b);
      al[s + 1] = pp_and_xor(al[s + 1], a1l, c.n1b);
      ah[s + 1] = pp_and_xor(ah[s + 1], a1h, c.n1b);
      bl[s + 1] = pp_and_xor(bl[s + 1], b1l, c.n1b);
      bh[s + 1] = pp_and_xor(bh[s + 1], b1h, c.n1b);
    }
  }
  prev0 = b.p0h;
  prev1 = b.p1h;
}

// The single-block form, as the loop of the launches with one member (G = 1) has it: the constants straight from the
// slots' row masks nb0[s] / nb1[s], one block per call.  The pair step equals two of these, a then b.
template <int Q, int NS>
SASSY_PP_HD void piece_block_step(const PiecePlanes& t, uint32_t& prev0, uint32_t& prev1, const uint32_t (&nb0)[NS], const uint32_t (&nb1)[NS],
                                  uint32_t (&al)[NS], uint32_t (&ah)[NS]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) al[s] = ah[s] = 0xFFFFFFFFu;
#pragma unroll
  for (int d = 0; d < Q; ++d) {
    const int j = Q - 1 - d;
    const uint32_t s0l = pp_shift_in(t.p0l, prev0, d), s0h = pp_shift_in(t.p0h, t.p0l, d);
    const uint32_t s1l = pp_shift_in(t.p1l, prev1, d), s1h = pp_shift_in(t.p1h, t.p1l, d);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const uint32_t n0 = pp_row_word(nb0[s], j), n1 = pp_row_word(nb1[s], j);
      al[s] = pp_and_xor(al[s], s0l, n0);
      ah[s] = pp_and_xor(ah[s], s0h, n0);
      al[s] = pp_and_xor(al[s], s1l, n1);
      ah[s] = pp_and_xor(ah[s], s1h, n1);
    }
  }
  prev0 = t.p0h;
  prev1 = t.p1h;
}

}  // namespace sassy_hip
