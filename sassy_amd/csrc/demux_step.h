// demux_step.h -- the arithmetic of demultiplexing a resident read batch (demux_reads.hip: sassy_hip_demux_reads), free of HIP
// and of the environment: plain C++17 that the device kernels and the host test driver (tests/c/demux_step_driver.cc) compile
// alike.  In the order of a call: what the call refuses, the barcode table, the window of a read, the planes of the window,
// the mismatches of one barcode, the combine of (cost, index) into best / second / n_best, the assignment rule, the clip
// window, the record, the bounds of a sample in the sorted labels.
//
// Read a of la bytes; barcodes p_0 .. p_{B-1} of ONE length m <= 64.  The window is the m bytes of the read at distance `at`
// from the chosen end; it is fetched as one 64-byte block (trim_step.h: trm_window_block, zero behind m) and packed into two
// words per plane (pairs_row_code per row, bit i of word w = row 32 w + i).  A barcode is two words per plane as well,
// wave-uniform; the rows that count are the m rows of the barcodes, one mask for the whole table.
#pragma once
#include <cstddef>
#include <cstdint>

#include "trim_step.h"

namespace sassy_hip {

constexpr uint32_t kDmxMaxBarcodes = 4096;   // SASSY_HIP_DEMUX_MAX_BARCODES
constexpr uint32_t kDmxMaxLen = 64;          // longest barcode: two words per plane
constexpr uint32_t kDmxMaxDelta = 65;        // a margin no pair of costs of 64 rows can miss
constexpr uint32_t kDmxEnd3 = 1u, kDmxKeepBarcode = 2u;  // SASSY_HIP_DEMUX_END3, SASSY_HIP_DEMUX_KEEP_BARCODE
constexpr uint32_t kDmxNoBest = 0xFFFFFFFFu; // `best` of a read without a window
// a barcode's entry of the table: word 2 p + w = word w of plane p; P planes
SASSY_HAM_HD uint32_t dmx_entry_words(uint32_t profile) { return 2u * ovl_planes(profile); }

// ---- what the call refuses, before any device work, in this order ----
struct DmxCall {
  bool have_searcher;
  uint32_t flags, min_delta, at;
  size_t n_barcodes, barcode_len;
  const uint8_t* const* barcodes;
  ReadsGate gate;                         // the searcher and the handle (reads_gate.h)
  bool have_bounds, have_sorted;          // out_bounds, out_sorted != NULL
};
enum DmxRefusal : uint32_t {
  kDmxOk = 0, kDmxNullSearcher, kDmxFlags, kDmxDelta, kDmxCount, kDmxLen, kDmxNullBarcode, kDmxAt, kDmxGate /* *gate says which */, kDmxNullOut
};
// *which: the barcode a refusal of the barcodes names.  The handle is read only once nothing in front of it is wrong.
inline DmxRefusal dmx_refusal(const DmxCall& c, size_t* which, ReadsRefusal* gate) {
  *which = 0;
  *gate = kRdsOk;
  if (!c.have_searcher) return kDmxNullSearcher;
  if (c.flags & ~(kDmxEnd3 | kDmxKeepBarcode)) return kDmxFlags;
  if (c.min_delta > kDmxMaxDelta) return kDmxDelta;
  if (c.n_barcodes == 0 || c.n_barcodes > kDmxMaxBarcodes) return kDmxCount;
  if (c.barcode_len == 0 || c.barcode_len > kDmxMaxLen) return kDmxLen;
  if (!c.barcodes) return kDmxNullBarcode;
  for (size_t j = 0; j < c.n_barcodes; ++j)
    if (!c.barcodes[j]) {
      *which = j;
      return kDmxNullBarcode;
    }
  if ((uint64_t)c.at + c.barcode_len > kOvlMaxLen) return kDmxAt;
  if ((*gate = reads_gate_searcher(c.gate)) != kRdsOk) return kDmxGate;
  if ((*gate = reads_gate_handles(c.gate)) != kRdsOk) return kDmxGate;
  if (!c.have_bounds || !c.have_sorted) return kDmxNullOut;
  if ((*gate = reads_gate_tickets(c.gate)) != kRdsOk) return kDmxGate;
  return kDmxOk;
}

// ---- the barcode table, made once on the host ----
inline void dmx_encode_barcode(uint32_t profile, const uint8_t* p, uint32_t m, uint32_t* out) {
  const uint32_t P = ovl_planes(profile);
  for (uint32_t i = 0; i < 2u * P; ++i) out[i] = 0;
  for (uint32_t t = 0; t < m; ++t) {
    const uint32_t code = pairs_row_code(profile, p[t]);
    for (uint32_t pl = 0; pl < P; ++pl) out[2 * pl + (t >> 5)] |= ((code >> pl) & 1u) << (t & 31u);
  }
}
// the rows of word w that a barcode of m rows has
SASSY_HAM_HD uint32_t dmx_row_mask(uint32_t m, uint32_t w) { return pairs_row_mask(m, w); }
// key bits of the sort: labels 0 .. B
SASSY_HAM_HD uint32_t dmx_key_bits(uint32_t n_barcodes) {
  uint32_t bits = 1;
  while (bits < 32u && (n_barcodes >> bits) != 0u) ++bits;
  return bits;
}

// ---- the window ----
SASSY_HAM_HD bool dmx_has_window(uint32_t la, uint32_t at, uint32_t m) { return at + m <= la; }
// its first byte within the read (a read with a window)
SASSY_HAM_HD uint32_t dmx_window(uint32_t la, uint32_t at, uint32_t m, bool end3) { return end3 ? la - at - m : at; }

// ---- the planes of the window: blk = its 64 bytes as sixteen words, zero behind m ----
template <int P>
SASSY_HAM_HD void dmx_planes(uint32_t profile, const uint32_t (&blk)[16], uint32_t (&rw)[P + 1][2]) {
#pragma unroll
  for (int p = 0; p <= P; ++p) rw[p][0] = rw[p][1] = 0u;
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    const uint32_t code = pairs_row_code(profile, (blk[t >> 2] >> (8 * (t & 3))) & 0xFFu);
#pragma unroll
    for (int p = 0; p < P; ++p) rw[p][t >> 5] |= ((code >> p) & 1u) << (t & 31);
  }
  rw[P][0] = rw[P][1] = 0xFFFFFFFFu;  // (every row of a window exists; the barcodes' rows are the mask)
}
// cost_j: rw = dmx_planes of the window, bc = the barcode's table entry, mask = dmx_row_mask of the two words.  The two
// mismatch words are one 64-bit word under one popcount.
template <int P, bool IUPAC>
SASSY_HAM_HD uint32_t dmx_mismatches(const uint32_t (&rw)[P + 1][2], const uint32_t* bc, const uint32_t (&mask)[2]) {
  uint32_t mw[2];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    uint32_t aw[P + 1], bw[P + 1];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      aw[p] = bc[2 * p + w];
      bw[p] = rw[p][w];
    }
    aw[P] = mask[w];
    bw[P] = rw[P][w];
    mw[w] = ovl_mismatch_word<P, IUPAC>(aw, bw);
  }
  return (uint32_t)__builtin_popcountll(((uint64_t)mw[1] << 32) | mw[0]);
}

// ---- best, second, n_best ----
// What a lane has seen of a set of barcodes: the smallest (cost, index), how many share that cost, and the smallest cost among
// the others.  n == 0: none seen.
struct DmxBest {
  uint32_t cost, best, second, n;
};
constexpr uint32_t kDmxNone = 0xFFFFFFFFu;
SASSY_HAM_HD DmxBest dmx_none() { return DmxBest{kDmxNone, kDmxNone, kDmxNone, 0u}; }
// one barcode: no other yet, so second = m + 1
SASSY_HAM_HD DmxBest dmx_one(uint32_t cost, uint32_t j, uint32_t m) { return DmxBest{cost, j, m + 1u, 1u}; }
// Two partial results over disjoint sets of barcodes.  (cost, index) is a total order and two barcodes never share an index, so
// the order of a reduction does not show.
SASSY_HAM_HD DmxBest dmx_combine(const DmxBest& x, const DmxBest& y) {
  const bool tie = x.cost == y.cost;
  const bool keep_x = (x.cost < y.cost) | (tie & (x.best < y.best));  // (| and & for || and &&: no branch)
  const uint32_t win_second = keep_x ? x.second : y.second, lose_cost = keep_x ? y.cost : x.cost;
  return DmxBest{keep_x ? x.cost : y.cost, keep_x ? x.best : y.best, win_second < lose_cost ? win_second : lose_cost,
                 tie ? x.n + y.n : (keep_x ? x.n : y.n)};
}

// ---- the assignment ----
SASSY_HAM_HD bool dmx_assigned(bool has_window, const DmxBest& b, uint32_t k, uint32_t min_delta) {
  return has_window & (b.n != 0u) & (b.cost <= k) & (b.second - b.cost >= min_delta);  // (second >= cost: no wrap)
}
// the key of the sort: the unassigned bin comes last
SASSY_HAM_HD uint32_t dmx_label(bool assigned, const DmxBest& b, uint32_t n_barcodes) { return assigned ? b.best : n_barcodes; }

// ---- what is kept of a read ----
struct DmxClip {
  uint32_t begin, len;
};
SASSY_HAM_HD DmxClip dmx_clip(uint32_t la, uint32_t at, uint32_t m, bool end3, bool keep_barcode, bool assigned) {
  const bool clip = assigned & !keep_barcode;
  const uint32_t cut = clip ? at + m : 0u;  // (an assigned read has a window: at + m <= la)
  return DmxClip{(clip & !end3) ? cut : 0u, la - cut};
}
// does a call's write need the shifted path?  Only a clip at the 5' end moves a window's begin.
SASSY_HAM_HD bool dmx_shifted(uint32_t flags) { return (flags & (kDmxEnd3 | kDmxKeepBarcode)) == 0u; }

// ---- the record: sassy_hip_ReadDemux as four words, one 16-byte store ----
struct DmxRecord {
  uint32_t sample, best, tail, index;  // sample: int32, -1 unassigned; tail: cost | second << 8 | n_best << 16
};
SASSY_HAM_HD DmxRecord dmx_record(bool has_window, bool assigned, const DmxBest& b) {
  return DmxRecord{assigned ? b.best : 0xFFFFFFFFu, has_window ? b.best : kDmxNoBest,
                   has_window ? (b.cost | (b.second << 8) | (b.n << 16)) : 0x0000FFFFu, 0u};
}
SASSY_HAM_HD uint32_t dmx_record_label(const DmxRecord& r, uint32_t n_barcodes) { return r.sample == 0xFFFFFFFFu ? n_barcodes : r.sample; }

// ---- the bounds: the first place of label s in the sorted labels (key(i): label of place i), n where none is as large ----
template <typename Key>
SASSY_HAM_HD uint64_t dmx_lower_bound(const Key& key, uint64_t n, uint32_t s) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (key(mid) < s) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace sassy_hip
