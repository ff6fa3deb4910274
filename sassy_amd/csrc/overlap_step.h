// overlap_step.h -- the arithmetic of the paired-end overlap call (read_overlaps.hip: sassy_hip_read_overlaps), free of HIP
// and of the environment: plain C++17 that the device kernel and the host test driver (tests/c/overlap_step_driver.cc)
// compile alike.  In the order of a call: what the call refuses, the complement of a byte, the planes of the two reads, the
// offset geometry, the mismatches of one offset word by word, the acceptance test, which of two offsets is better and the
// combine rule of two partial results.
//
// Pair r: a = read r of R1 (la bytes), b = the reverse complement of read r of R2 (lb bytes), both at most kOvlMaxLen.  The
// offset d, -(lb - 1) <= d <= la - 1, places b[0] under a[d]; the two overlap in the rows [lo, hi) of a, lo = max(0, d),
// hi = min(la, d + lb), ov = hi - lo, and mm(d) = #{ i in [lo, hi) : !ham_match(profile, a[i], b[i - d]) }.
//
// A read becomes bit planes of 32-bit words as in pairs_step.h (pairs_row_code: Dna 2 planes under xor, Iupac 4 under and)
// and one more plane, VALID, whose bit t says "row t exists".  Bit i of word w of a plane is row 32 w + i.  b's planes
// stand in the middle third of an array of 3 W words per plane whose outer thirds are zero: the words of b shifted to offset
// d are then a funnel shift of two neighbouring words at one word index per offset, for every d, with no bound to test.  The
// rows of the overlap in word w are valid_a[w] & shifted valid_b[w] -- the range mask: under xor a row outside of it would
// count against b's zero pad, under Iupac the complement of the match word would.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pairs_step.h"
#include "reads_gate.h"

namespace sassy_hip {

constexpr uint32_t kOvlMaxLen = 512;     // longest read (SASSY_HIP_OVERLAP_MAX_LEN): 16 words per plane
static_assert(kOvlMaxLen == kReadsMaxLen, "the gate refuses what the kernels do not take");
constexpr uint32_t kOvlMaxWords = kOvlMaxLen / 32;
constexpr uint32_t kOvlWave = 64;        // offsets of a round: one per lane
constexpr uint32_t kOvlPairsPerGroup = 4;  // pairs of a workgroup: one per wavefront

// words per plane the kernel is instantiated for: 2, 4, 6, 8 or 16 (reads of at most 64, 128, 192, 256, 512 bytes)
SASSY_HAM_HD uint32_t ovl_words(uint32_t longest) {
  return longest <= 64 ? 2u : longest <= 128 ? 4u : longest <= 192 ? 6u : longest <= 256 ? 8u : kOvlMaxWords;
}
SASSY_HAM_HD uint32_t ovl_planes(uint32_t profile) { return profile == kHamIupac ? 4u : 2u; }

// ---- what the call refuses, before any device work, in this order ----
struct OvlCall {
  bool have_searcher, have_out;
  uint32_t min_overlap, max_permille, flags;
  uint64_t n1, n2;                           // of the handles
  ReadsGate gate;                            // the searcher and the two handles (reads_gate.h)
};
enum OvlRefusal : uint32_t { kOvlOk = 0, kOvlNullSearcher, kOvlFlags, kOvlMinOverlap, kOvlPermille, kOvlGate /* *gate says which */, kOvlCounts, kOvlNullOut };
// The searcher and the numbers first, then the handles, then what is read out of the handles.  Zero pairs need no `out`.
// (The tickets come behind all of it, in the entry points.)
SASSY_HAM_HD OvlRefusal ovl_refusal(const OvlCall& c, ReadsRefusal* gate) {
  *gate = kRdsOk;
  if (!c.have_searcher) return kOvlNullSearcher;
  if (c.flags) return kOvlFlags;
  if (c.min_overlap == 0) return kOvlMinOverlap;
  if (c.max_permille > 1000) return kOvlPermille;
  if ((*gate = reads_gate_searcher(c.gate)) != kRdsOk) return kOvlGate;
  if (c.n1 != c.n2) return kOvlCounts;
  if ((*gate = reads_gate_handles(c.gate)) != kRdsOk) return kOvlGate;
  if (c.n1 && !c.have_out) return kOvlNullOut;
  return kOvlOk;
}

// ---- the complement of one byte: profiles.h's complement_char, per byte, for the device ----
// Dna: upper-case A, C, G, T only.  Iupac: the IUPAC letters in both cases, the case kept; U is no letter of the table and
// stays U (it matches as T, its complement does too); what is no letter stays as it is.
SASSY_HAM_HD uint32_t ovl_complement(uint32_t profile, uint32_t c) {
  // (selects, no branches: the kernel complements 64 bytes a step, one per lane)
  if (profile == kHamDna) return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'T' ? 'A' : c == 'G' ? 'C' : c;
  const uint32_t up = c & ~0x20u, low = c & 0x20u;
  const uint32_t to = up == 'A' ? 'T' : up == 'C' ? 'G' : up == 'T' ? 'A' : up == 'G' ? 'C' : up == 'R' ? 'Y' : up == 'Y' ? 'R' : up == 'K' ? 'M'
                    : up == 'M' ? 'K' : up == 'B' ? 'V' : up == 'D' ? 'H' : up == 'H' ? 'D' : up == 'V' ? 'B' : 0u;
  return to ? (to | low) : c;  // (S, W, N, X are their own complements; so is everything that is no letter)
}
// what the planes of row t of a (strand 0) or of b (strand 1: the byte is R2's, read from its far end) say
SASSY_HAM_HD uint32_t ovl_row_code(uint32_t profile, uint32_t c, uint32_t strand) {
  return pairs_row_code(profile, strand ? ovl_complement(profile, c) : c);
}

// ---- the planes on the host (the kernel builds the same words from ballots, 64 rows at a time) ----
// a: out[p * W + w], p < P the code planes, p == P the VALID plane; rows >= la are zero in every plane
inline void ovl_encode_a(uint32_t profile, const uint8_t* a, uint32_t la, uint32_t W, uint32_t* out) {
  const uint32_t P = ovl_planes(profile);
  for (uint32_t i = 0; i < (P + 1) * W; ++i) out[i] = 0;
  for (uint32_t t = 0; t < la; ++t) {
    const uint32_t code = ovl_row_code(profile, a[t], 0);
    for (uint32_t p = 0; p < P; ++p) out[p * W + (t >> 5)] |= ((code >> p) & 1u) << (t & 31u);
    out[P * W + (t >> 5)] |= 1u << (t & 31u);
  }
}
// b out of R2's read r2[0 .. lb): out[p * 3 W + W + w], the outer thirds zero
inline void ovl_encode_b(uint32_t profile, const uint8_t* r2, uint32_t lb, uint32_t W, uint32_t* out) {
  const uint32_t P = ovl_planes(profile);
  for (uint32_t i = 0; i < (P + 1) * 3 * W; ++i) out[i] = 0;
  for (uint32_t t = 0; t < lb; ++t) {
    const uint32_t code = ovl_row_code(profile, r2[lb - 1 - t], 1);
    for (uint32_t p = 0; p < P; ++p) out[p * 3 * W + W + (t >> 5)] |= ((code >> p) & 1u) << (t & 31u);
    out[P * 3 * W + W + (t >> 5)] |= 1u << (t & 31u);
  }
}

// ---- the offsets ----
// The offsets a call looks at are those whose overlap can be accepted, ov >= min_overlap (>= 1): d_first .. d_first + count - 1,
// a part of -(lb - 1) .. la - 1.  No such offset (a read shorter than min_overlap, an empty read): count == 0.
struct OvlRange {
  int32_t d_first;
  uint32_t count;
};
SASSY_HAM_HD OvlRange ovl_offsets(uint32_t la, uint32_t lb, uint32_t min_overlap) {
  if (la < min_overlap || lb < min_overlap || min_overlap == 0) return OvlRange{0, 0u};
  return OvlRange{-(int32_t)(lb - min_overlap), la + lb - 2u * min_overlap + 1u};
}
SASSY_HAM_HD uint32_t ovl_rounds(uint32_t count) { return (count + kOvlWave - 1) / kOvlWave; }
SASSY_HAM_HD int32_t ovl_lo(int32_t d) { return d > 0 ? d : 0; }
SASSY_HAM_HD int32_t ovl_hi(uint32_t la, uint32_t lb, int32_t d) { return (int32_t)la < d + (int32_t)lb ? (int32_t)la : d + (int32_t)lb; }
SASSY_HAM_HD uint32_t ovl_overlap(uint32_t la, uint32_t lb, int32_t d) {
  const int32_t ov = ovl_hi(la, lb, d) - ovl_lo(d);
  return ov > 0 ? (uint32_t)ov : 0u;
}
// Where offset d finds b's words in the padded array: word w of the shifted plane is bits [r, r + 32) of the two words at
// q + w and q + w + 1, q = W + floor(-d / 32), r = (-d) mod 32.  |d| < 32 W: 0 <= q and q + W <= 3 W - 1.
SASSY_HAM_HD uint32_t ovl_shift_word(uint32_t W, int32_t d) { return (uint32_t)((int32_t)W + ((-d) >> 5)); }
SASSY_HAM_HD uint32_t ovl_shift_bits(int32_t d) { return (uint32_t)(-d) & 31u; }
// bits [r, r + 32) of hi:lo, 0 <= r < 32 (the kernel: one v_alignbit_b32)
SASSY_HAM_HD uint32_t ovl_funnel(uint32_t lo, uint32_t hi, uint32_t r) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> r); }
// word w of plane `plane` of b at offset (q, r); bpad: the padded planes, 3 W words each
SASSY_HAM_HD uint32_t ovl_shifted_word(const uint32_t* bpad, uint32_t W, uint32_t plane, uint32_t q, uint32_t r, uint32_t w) {
  const uint32_t* at = bpad + plane * 3u * W + q + w;
  return ovl_funnel(at[0], at[1], r);
}
// The mismatching rows of word w at one offset.  a[p]: word w of a's plane p (p == P: VALID); b[p]: the shifted word of
// b's plane p.  The range mask is a[P] & b[P].
template <int P, bool IUPAC>
SASSY_HAM_HD uint32_t ovl_mismatch_word(const uint32_t* a, const uint32_t* b) {
  uint32_t acc = 0;
#pragma unroll
  for (int p = 0; p < P; ++p) acc |= IUPAC ? (a[p] & b[p]) : (a[p] ^ b[p]);
  return (IUPAC ? ~acc : acc) & a[P] & b[P];
}
// mm(d) from the planes: a as ovl_encode_a lays it out, bpad as ovl_encode_b does
template <int P, bool IUPAC>
inline uint32_t ovl_mismatches(const uint32_t* a, const uint32_t* bpad, uint32_t W, int32_t d) {
  const uint32_t q = ovl_shift_word(W, d), r = ovl_shift_bits(d);
  uint32_t mm = 0;
  for (uint32_t w = 0; w < W; ++w) {
    uint32_t aw[P + 1], bw[P + 1];
    for (uint32_t p = 0; p <= (uint32_t)P; ++p) {
      aw[p] = a[p * W + w];
      bw[p] = ovl_shifted_word(bpad, W, p, q, r, w);
    }
    mm = pairs_popcount(ovl_mismatch_word<P, IUPAC>(aw, bw), mm);
  }
  return mm;
}

// ---- acceptance, in integers: mm <= 512 and ov <= 512, so every product fits 32 bits ----
SASSY_HAM_HD bool ovl_accepts(uint32_t mm, uint32_t ov, uint32_t min_overlap, uint32_t k, uint32_t max_permille) {
  return (ov >= min_overlap) & (mm <= k) & (mm * 1000u <= max_permille * ov);  // (& for &&: nothing to skip, no branch)
}

// ---- the best offset and the number of accepted ones ----
// What a lane, a wavefront or a pair has seen: the best accepted offset so far and how many were accepted.  n == 0: none,
// and the other fields are zero -- which is the record of a pair without an overlap.
struct OvlBest {
  int32_t d;
  uint32_t ov, mm, n;
};
SASSY_HAM_HD OvlBest ovl_none() { return OvlBest{0, 0u, 0u, 0u}; }
// FLASH's rule with the ties fixed: the lower mismatch density mm / ov (cross-multiplied); at equal density the longer
// overlap; at equal overlap the larger d.  Two different offsets never tie, so the order of a reduction does not show.
SASSY_HAM_HD bool ovl_better(uint32_t mm1, uint32_t ov1, int32_t d1, uint32_t mm2, uint32_t ov2, int32_t d2) {
  const uint32_t x = mm1 * ov2, y = mm2 * ov1;
  return (x < y) | ((x == y) & ((ov1 > ov2) | ((ov1 == ov2) & (d1 > d2))));  // (| and & for || and &&: no branch)
}
// two partial results over disjoint sets of offsets
SASSY_HAM_HD OvlBest ovl_combine(const OvlBest& x, const OvlBest& y) {
  const bool keep_x = (y.n == 0) | ((x.n != 0) & ovl_better(x.mm, x.ov, x.d, y.mm, y.ov, y.d));  // (field by field: selects, no memory)
  return OvlBest{keep_x ? x.d : y.d, keep_x ? x.ov : y.ov, keep_x ? x.mm : y.mm, x.n + y.n};
}
// one offset as a partial result
SASSY_HAM_HD OvlBest ovl_one(int32_t d, uint32_t ov, uint32_t mm, bool accepted) { return accepted ? OvlBest{d, ov, mm, 1u} : ovl_none(); }

}  // namespace sassy_hip
