// trim_step.h -- the arithmetic of adapter and quality trimming (trim_reads.hip: sassy_hip_trim_reads, sassy_hip_reads_slice),
// free of HIP and of the environment: plain C++17 that the device kernels and the host test driver
// (tests/c/trim_step_driver.cc) compile alike.  In the order of a call: what the call refuses, the adapter table, the quality
// walk as a wavefront does it, the planes of a read, the positions, the mismatches of one position, which of two positions
// is better and the combine rule, the record, and one 64-byte block of a window of a read.
//
// Read a of la bytes (at most kOvlMaxLen) with qualities q; adapters p_j of m_j <= 64 bytes.  The roles of overlap_step.h
// swap: the READ becomes bit planes in LDS (pairs_row_code per row, bit i of word w = row 32 w + i) with a VALID plane cut at
// lq and two zero words behind every plane; an ADAPTER is two words per plane, wave-uniform.  Position c places p_j[0] under
// a[c]: the read's rows c .. c + 63 are a funnel shift of three neighbouring words by c mod 32, and the rows that count are
// VALID's shifted word & the adapter's own valid word.
#pragma once
#include <cstddef>
#include <cstdint>

#include "fastq_step.h"
#include "overlap_step.h"

namespace sassy_hip {

constexpr uint32_t kTrmMaxAdapters = 64;     // SASSY_HIP_TRIM_MAX_ADAPTERS
constexpr uint32_t kTrmMaxAdapterLen = 64;   // two words per plane
constexpr uint32_t kTrmMaxCutoff = 93;       // Phred+33 in printable bytes
constexpr uint32_t kTrmReadsPerGroup = 4;    // reads of a workgroup: one per wavefront
constexpr uint32_t kTrmPad = 2;              // zero words behind a plane of the read
// an adapter's entry of the table: word 2 p + w = word w of plane p (p == P: its valid rows), word kTrmLenWord = m_j
constexpr uint32_t kTrmTableWords = 12, kTrmLenWord = 10;

// ---- what the call refuses, before any device work, in this order ----
struct TrmCall {
  bool have_searcher;
  uint32_t flags, min_overlap, max_permille, quality_cutoff;
  const uint8_t* const* adapters;
  const size_t* adapter_lens;
  size_t n_adapters;
  ReadsGate gate;                         // the searcher and the handle (reads_gate.h)
  bool kept_quality;                      // read with the gate's handle fields
  bool have_trimmed;                      // out_trimmed != NULL
};
enum TrmRefusal : uint32_t {
  kTrmOk = 0, kTrmNullSearcher, kTrmFlags, kTrmMinOverlap, kTrmPermille, kTrmCutoff, kTrmTooMany, kTrmNullAdapter, kTrmEmptyAdapter,
  kTrmLongAdapter, kTrmShortAdapter, kTrmGate /* *gate says which */, kTrmNoQuality, kTrmNullTrimmed
};
// *which: the adapter a refusal of the adapters names.  The handle is read only once nothing in front of it is wrong.
inline TrmRefusal trm_refusal(const TrmCall& c, size_t* which, ReadsRefusal* gate) {
  *which = 0;
  *gate = kRdsOk;
  if (!c.have_searcher) return kTrmNullSearcher;
  if (c.flags) return kTrmFlags;
  if (c.min_overlap == 0) return kTrmMinOverlap;
  if (c.max_permille > 1000) return kTrmPermille;
  if (c.quality_cutoff > kTrmMaxCutoff) return kTrmCutoff;
  if (c.n_adapters > kTrmMaxAdapters) return kTrmTooMany;
  if (c.n_adapters && (!c.adapters || !c.adapter_lens)) return kTrmNullAdapter;
  for (size_t j = 0; j < c.n_adapters; ++j) {
    *which = j;
    if (!c.adapters[j]) return kTrmNullAdapter;
    if (c.adapter_lens[j] == 0) return kTrmEmptyAdapter;
    if (c.adapter_lens[j] > kTrmMaxAdapterLen) return kTrmLongAdapter;
    if (c.adapter_lens[j] < c.min_overlap) return kTrmShortAdapter;
  }
  *which = 0;
  if ((*gate = reads_gate_searcher(c.gate)) != kRdsOk) return kTrmGate;
  if ((*gate = reads_gate_handles(c.gate)) != kRdsOk) return kTrmGate;
  if (c.gate.handle_read && c.quality_cutoff && !c.kept_quality) return kTrmNoQuality;
  if (!c.have_trimmed) return kTrmNullTrimmed;
  if ((*gate = reads_gate_tickets(c.gate)) != kRdsOk) return kTrmGate;
  return kTrmOk;
}

// ---- the adapter table, made once on the host ----
inline void trm_encode_adapter(uint32_t profile, const uint8_t* p, uint32_t m, uint32_t* out) {
  const uint32_t P = ovl_planes(profile);
  for (uint32_t i = 0; i < kTrmTableWords; ++i) out[i] = 0;
  for (uint32_t t = 0; t < m; ++t) {
    const uint32_t code = pairs_row_code(profile, p[t]);
    for (uint32_t pl = 0; pl < P; ++pl) out[2 * pl + (t >> 5)] |= ((code >> pl) & 1u) << (t & 31u);
    out[2 * P + (t >> 5)] |= 1u << (t & 31u);
  }
  out[kTrmLenWord] = m;
}

// ---- the quality walk, 64 bytes a round from the read's far end, a lane per byte ----
SASSY_HAM_HD int32_t trm_term(uint32_t q, uint32_t cutoff) { return (int32_t)q - 33 - (int32_t)cutoff; }
// one step of the inclusive suffix scan over a wavefront: `other` is the value of lane + o
SASSY_HAM_HD int32_t trm_scan_add(int32_t incl, int32_t other, uint32_t lane, uint32_t o) { return lane + o < 64u ? incl + other : incl; }
// the highest lane of a round whose sum is positive (pos: the ballot), -1 where none is: the walk stops there, and the lanes
// above it are the ones it has looked at
SASSY_HAM_HD int32_t trm_stop_lane(uint64_t pos) {
  int32_t top = -1;
#pragma unroll
  for (int b = 32; b >= 1; b >>= 1) {
    const bool up = (pos >> b) != 0;
    top += up ? b : 0;
    pos = up ? pos >> b : pos;
  }
  return pos ? top + 1 : -1;
}
// the lowest sum seen and its row; s == 0: none was below zero
struct TrmLow {
  int32_t s;
  uint32_t i;
};
SASSY_HAM_HD TrmLow trm_low_none(uint32_t la) { return TrmLow{0, la}; }
// a lane meets row i with sum s: strictly smaller only (its rows descend, so a tie stays with the larger row)
SASSY_HAM_HD TrmLow trm_low_take(const TrmLow& x, int32_t s, uint32_t i, bool looked_at) {
  const bool take = looked_at & (s < x.s);
  return TrmLow{take ? s : x.s, take ? i : x.i};
}
// two lanes: the smaller sum, at equal sums the larger row
SASSY_HAM_HD TrmLow trm_low_combine(const TrmLow& x, const TrmLow& y) {
  const bool keep_x = (x.s < y.s) | ((x.s == y.s) & (x.i >= y.i));
  return TrmLow{keep_x ? x.s : y.s, keep_x ? x.i : y.i};
}
SASSY_HAM_HD uint32_t trm_quality_len(const TrmLow& low, uint32_t la) { return low.s < 0 ? low.i : la; }

// ---- the planes of the read on the host (the kernel builds the same words from ballots, 64 rows at a time) ----
// out[p * (W + kTrmPad) + w], p < P the code planes of a[0 .. la), p == P the VALID plane: rows below lq
inline void trm_encode_read(uint32_t profile, const uint8_t* a, uint32_t la, uint32_t lq, uint32_t W, uint32_t* out) {
  const uint32_t P = ovl_planes(profile), S = W + kTrmPad;
  for (uint32_t i = 0; i < (P + 1) * S; ++i) out[i] = 0;
  for (uint32_t t = 0; t < la; ++t) {
    const uint32_t code = pairs_row_code(profile, a[t]);
    for (uint32_t p = 0; p < P; ++p) out[p * S + (t >> 5)] |= ((code >> p) & 1u) << (t & 31u);
    if (t < lq) out[P * S + (t >> 5)] |= 1u << (t & 31u);
  }
}

// ---- the positions ----
// those whose overlap can be accepted: 0 .. lq - min_overlap (every adapter is at least min_overlap long)
SASSY_HAM_HD uint32_t trm_positions(uint32_t lq, uint32_t min_overlap) { return lq >= min_overlap && min_overlap ? lq - min_overlap + 1u : 0u; }
SASSY_HAM_HD uint32_t trm_overlap(uint32_t m, uint32_t lq, uint32_t c) { return m < lq - c ? m : lq - c; }
// rows c .. c + 63 of one plane of the read as two words: c < 32 W, so the three words lie inside the plane and its pad
SASSY_HAM_HD void trm_window(const uint32_t* plane, uint32_t c, uint32_t (&out)[2]) {
  const uint32_t q = c >> 5, r = c & 31u;
  out[0] = ovl_funnel(plane[q], plane[q + 1], r);
  out[1] = ovl_funnel(plane[q + 1], plane[q + 2], r);
}
// mm(c, j): rw[p] = trm_window of plane p (p == P: VALID), ad = the adapter's table entry
template <int P, bool IUPAC>
SASSY_HAM_HD uint32_t trm_mismatches(const uint32_t (&rw)[P + 1][2], const uint32_t* ad) {
  uint32_t mm = 0;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    uint32_t aw[P + 1], bw[P + 1];
#pragma unroll
    for (int p = 0; p <= P; ++p) {
      aw[p] = ad[2 * p + w];
      bw[p] = rw[p][w];
    }
    mm = pairs_popcount(ovl_mismatch_word<P, IUPAC>(aw, bw), mm);
  }
  return mm;
}

// ---- the best position ----
struct TrmBest {
  uint32_t c, ov, mm, j, found;  // found == 0: none, and the other fields are zero
};
SASSY_HAM_HD TrmBest trm_none() { return TrmBest{0u, 0u, 0u, 0u, 0u}; }
// the smaller c; at equal c the lower density (cross-multiplied; mm, ov <= 64); at equal density the larger ov; at equal ov
// the smaller j.  Two different (c, j) never tie, so the order of a reduction does not show.
SASSY_HAM_HD bool trm_better(uint32_t c1, uint32_t mm1, uint32_t ov1, uint32_t j1, uint32_t c2, uint32_t mm2, uint32_t ov2, uint32_t j2) {
  const uint32_t x = mm1 * ov2, y = mm2 * ov1;
  return (c1 < c2) | ((c1 == c2) & ((x < y) | ((x == y) & ((ov1 > ov2) | ((ov1 == ov2) & (j1 < j2))))));  // (| and & for || and &&: no branch)
}
SASSY_HAM_HD TrmBest trm_combine(const TrmBest& x, const TrmBest& y) {
  const bool keep_x = (y.found == 0) | ((x.found != 0) & trm_better(x.c, x.mm, x.ov, x.j, y.c, y.mm, y.ov, y.j));  // (field by field: selects)
  return TrmBest{keep_x ? x.c : y.c, keep_x ? x.ov : y.ov, keep_x ? x.mm : y.mm, keep_x ? x.j : y.j, x.found | y.found};
}
SASSY_HAM_HD TrmBest trm_one(uint32_t c, uint32_t ov, uint32_t mm, uint32_t j, bool accepted) {
  return TrmBest{accepted ? c : 0u, accepted ? ov : 0u, accepted ? mm : 0u, accepted ? j : 0u, accepted ? 1u : 0u};
}

// ---- the record: sassy_hip_ReadTrim as four words, one 16-byte store ----
struct TrmRecord {
  uint32_t length, quality_len, adapter_pos, tail;  // tail: adapter (int16) | overlap << 16 | mismatches << 24
};
SASSY_HAM_HD TrmRecord trm_record(const TrmBest& best, uint32_t lq, uint32_t min_length) {
  const uint32_t cut = best.found ? best.c : lq;
  const uint32_t adapter = best.found ? best.j : 0xFFFFu;
  return TrmRecord{cut >= min_length ? cut : 0u, lq, cut, adapter | (best.ov << 16) | (best.mm << 24)};
}

// ---- one 64-byte block of a window: bytes src .. src + 63 of a buffer of `bytes` bytes (a multiple of 16) ----
// Five 16-byte pieces from src rounded down to 16, each loaded only where it begins inside the buffer (load16(at, w): four
// words from byte `at`), shifted by fq_shift_block; bytes at or behind `keep` are zero.
#if defined(__HIPCC__)
// load16 over a device buffer, for the kernels: one 16-byte load (at: a multiple of 16)
struct TrmLoad16 {
  const uint8_t* base;
  __device__ __forceinline__ void operator()(uint64_t at, uint32_t* w) const {
    const uint4 v = *reinterpret_cast<const uint4*>(base + at);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  }
};
#endif
template <typename Load16>
SASSY_HAM_HD void trm_window_block(const Load16& load16, uint64_t src, uint64_t bytes, uint32_t keep, uint32_t (&out)[16]) {
  const uint64_t al = src & ~15ull;
  uint32_t w[20];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const uint64_t at = al + 16u * j;
    w[4 * j] = w[4 * j + 1] = w[4 * j + 2] = w[4 * j + 3] = 0u;
    if (at < bytes) load16(at, &w[4 * j]);
  }
  fq_shift_block(w, (uint32_t)(src & 15ull), keep, out);
}

// Quarter q (bytes 16 q .. 16 q + 15) of the block where src is a multiple of 16 (a trim: the window begins its read, a read
// starts at a multiple of 64): one piece, loaded only where it begins inside the buffer, zero at or behind `keep`.
template <typename Load16>
SASSY_HAM_HD void trm_aligned_quarter(const Load16& load16, uint64_t src, uint64_t bytes, uint32_t keep, uint32_t q, uint32_t (&out)[4]) {
  const uint64_t at = src + 16u * q;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (at < bytes && keep > 16u * q) load16(at, w);
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t first = 16u * q + 4u * j, left = keep > first ? keep - first : 0u;  // bytes of this word that are kept
    out[j] = left >= 4u ? w[j] : (w[j] & ((1u << (8u * left)) - 1u));
  }
}

}  // namespace sassy_hip
