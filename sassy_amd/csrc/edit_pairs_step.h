// edit_pairs_step.h -- the arithmetic of the all-vs-all edit-distance calls (edit_pairs.hip: sassy_hip_edit_pairs and
// sassy_hip_edit_nearest), free of HIP and of the environment: plain C++17 that the device kernels and the host test driver
// (tests/c/edit_pairs_step_driver.cc) compile alike.  The cells, the plan and the self-mode triangle are pairs_step.h's.
//
// E(x, y): the Levenshtein distance of x (m_a rows) and y (m_b columns), 1 <= m_a, m_b <= 64, under the profile relation of
// the Hamming family (hamming_step.h: ham_match); both are consumed whole, D[0][j] = j and D[i][0] = i.
//   x  an entry of A: pairs_encode's bit planes as they are, P planes of W = pairs_words(m_a) <= 2 words
//   y  a target record: one row code per column (pairs_row_code, P bits), 32 / P columns to a word, column 0 lowest
// A lane keeps the vertical deltas of its entry against a record as two bit vectors Pv / Mv and steps them one column at a
// time (Myers' bit-vector step as revised by Hyyro, with the global carry: the horizontal delta above row 0 is +1).  The Eq
// word of a column comes straight from the planes and the column's code, which is the same for every lane of a wavefront:
//   Dna, Ascii   rows where every plane bit equals the code bit    Eq = AND_p ~(a_p ^ c_p)      c_p = bit p of the code, spread
//   Iupac        rows where the sets meet                          Eq = OR_p (a_p & c_p)
// No per-symbol table and no row mask inside the walk: no bit of the step influences a lower one, so what rows m_a .. 32 W - 1
// hold is never read.  The score is not carried along either: after column m_b the vertical deltas are all there, and
//   E = D[m_a][m_b] = D[0][m_b] + sum_i (D[i][m_b] - D[i-1][m_b]) = m_b + popcount(Pv & rows) - popcount(Mv & rows)
// which takes the two bit tests, the add and the subtract per column out of the walk.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "pairs_step.h"

namespace sassy_hip {

constexpr uint32_t kEditMaxRows = 64;  // longest sequence of either list: 2 words per plane
// edit_pairs' finest chunk of targets (pairs_plan's fine_chunk): a pair costs some 50 times the Hamming walk's, so staging a
// tile weighs nothing and chunks an eighth of kPairsFineChunk even out the self-mode triangle and shorten the fill's walks
constexpr uint64_t kEditFineChunk = 2048;

// the bit vector of W words
template <int W>
using EditWord = typename std::conditional<W == 1, uint32_t, uint64_t>::type;

// columns of a record per word, words per record
SASSY_HAM_HD uint32_t edit_cols_per_word(uint32_t P) { return 32u / P; }
SASSY_HAM_HD uint32_t edit_record_words(uint32_t P, uint32_t m_b) { return (m_b * P + 31u) / 32u; }
// out[0 .. edit_record_words): the row codes of seq[0 .. m_b)
inline void edit_encode_record(uint32_t profile, const uint8_t* seq, uint32_t m_b, uint32_t* out) {
  const uint32_t P = pairs_planes(profile), cpw = edit_cols_per_word(P), rw = edit_record_words(P, m_b);
  for (uint32_t w = 0; w < rw; ++w) out[w] = 0u;
  for (uint32_t j = 0; j < m_b; ++j) out[j / cpw] |= pairs_row_code(profile, seq[j]) << (P * (j % cpw));
}
// the code of column j of an encoded record
SASSY_HAM_HD uint32_t edit_record_code(uint32_t P, const uint32_t* rec, uint32_t j) {
  const uint32_t cpw = edit_cols_per_word(P);
  return (rec[j / cpw] >> (P * (j % cpw))) & ((1u << P) - 1u);
}

// the planes of an entry (pairs_encode: plane p's word w at [p * W + w]) as P bit vectors
template <int P, int W>
SASSY_HAM_HD void edit_entry_planes(const uint32_t* planes, EditWord<W> (&a)[P]) {
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if constexpr (W == 1) a[p] = planes[p];
    else a[p] = (uint64_t)planes[p * 2] | ((uint64_t)planes[p * 2 + 1] << 32);
  }
}

// the rows of the entry that match a column of code `code` (the low P bits are read)
template <int P, int W, bool IUPAC>
SASSY_HAM_HD EditWord<W> edit_eq(const EditWord<W> (&a)[P], uint32_t code) {
  using Word = EditWord<W>;
  Word acc = IUPAC ? (Word)0 : ~(Word)0;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const Word c = (Word)0 - (Word)((code >> p) & 1u);  // bit p of the code on every row
    if (IUPAC) acc |= a[p] & c;
    else acc &= ~(a[p] ^ c);
  }
  return acc;
}

// One column: the vertical deltas Pv / Mv of column j - 1 become those of column j.  Start: Pv = all rows, Mv = none
// (D[i][0] = i).  W = 2 carries the addition and the two shifts across the word border inside the 64-bit operations.
template <int W>
SASSY_HAM_HD void edit_column(EditWord<W> eq, EditWord<W>& Pv, EditWord<W>& Mv) {
  using Word = EditWord<W>;
  const Word Xv = eq | Mv;
  const Word Xh = (((eq & Pv) + Pv) ^ Pv) | eq;
  Word Ph = Mv | ~(Xh | Pv);
  const Word Mh = Pv & Xh;
  Ph = (Ph << 1) | (Word)1;  // (the global boundary: D[0][j] - D[0][j - 1] = +1)
  Pv = (Mh << 1) | ~(Xv | Ph);
  Mv = Ph & Xv;
}

template <int W>
SASSY_HAM_HD EditWord<W> edit_rows(uint32_t m_a) {
  return m_a >= 32u * W ? ~(EditWord<W>)0 : ((EditWord<W>)1 << m_a) - (EditWord<W>)1;
}
SASSY_HAM_HD uint32_t edit_popcount(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
SASSY_HAM_HD uint32_t edit_popcount(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
// E after m_b columns, from the vertical deltas of the last one; rows = edit_rows<W>(m_a)
template <int W>
SASSY_HAM_HD uint32_t edit_score(EditWord<W> Pv, EditWord<W> Mv, EditWord<W> rows, uint32_t m_b) {
  return m_b + edit_popcount(Pv & rows) - edit_popcount(Mv & rows);
}

// E of an entry's planes and an encoded record: what one lane computes for one pair
template <int P, int W, bool IUPAC>
SASSY_HAM_HD uint32_t edit_cost(const uint32_t* planes, const uint32_t* rec, uint32_t m_a, uint32_t m_b) {
  EditWord<W> a[P], Pv = ~(EditWord<W>)0, Mv = 0;
  edit_entry_planes<P, W>(planes, a);
  for (uint32_t j = 0; j < m_b; ++j) edit_column<W>(edit_eq<P, W, IUPAC>(a, edit_record_code(P, rec, j)), Pv, Mv);
  return edit_score<W>(Pv, Mv, edit_rows<W>(m_a), m_b);
}

}  // namespace sassy_hip
