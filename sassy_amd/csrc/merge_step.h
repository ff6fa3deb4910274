// merge_step.h -- the arithmetic of the paired-end merge (merge_pairs.hip: sassy_hip_merge_pairs), free of HIP and of the
// environment: plain C++17 that the device kernels and the host test driver (tests/c/merge_step_driver.cc) compile alike.
// In the order of a call: what the call refuses, the merged length of a pair, which reads cover a column, the consensus of a
// column, and one word (four columns) of the merged read as the write kernel builds it.
//
// Pair r: a = read r of R1 with qualities qa (la bytes), b = the reverse complement of read r of R2 (lb bytes; ovl_complement
// per byte, read from the far end) with R2's qualities reversed, qb.  rec = the pair's overlap record (d, ov, mm, n_accepted;
// overlap_step.h).  n_accepted == 0: the pair is not merged, its merged read is empty.  Otherwise the merged read has
// L = max(la, d + lb) columns for d >= 0 and L = ov for d < 0 (read-through: R2's head and R1's tail beyond it are adapter
// and are dropped); column p, 0 <= p < L, is row i = p of a where i < la and row j = p - d of b where 0 <= j < lb.
#pragma once
#include <cstddef>
#include <cstdint>

#include "overlap_step.h"

namespace sassy_hip {

// ---- what the call refuses, before any device work, in this order ----
// Everything read_overlaps refuses, through its own function (the records need no host buffer: have_out is the caller's
// to set), then what the merge adds: both handles keep their qualities, and there is a place for the new handle.
struct MrgCall {
  OvlCall ovl;
  bool qual1, qual2;       // the handles own a quality buffer (SASSY_HIP_KEEP_QUALITY); read with the gate's handle fields
  bool have_merged;        // out_merged != NULL
};
enum MrgRefusal : uint32_t { kMrgOk = 0, kMrgOverlap /* *why says which, and *gate where that is kOvlGate */, kMrgNoQuality, kMrgNullMerged };
SASSY_HAM_HD MrgRefusal mrg_refusal(const MrgCall& c, OvlRefusal* why, ReadsRefusal* gate) {
  *why = ovl_refusal(c.ovl, gate);
  if (*why != kOvlOk) return kMrgOverlap;
  if (c.ovl.gate.handle_read && (!c.qual1 || !c.qual2)) return kMrgNoQuality;
  if (!c.have_merged) return kMrgNullMerged;
  return kMrgOk;
}

// ---- the merged length: overlap_trims' insert ----
SASSY_HAM_HD uint32_t mrg_length(uint32_t la, uint32_t lb, const OvlBest& rec) {
  const uint32_t ext = (uint32_t)rec.d + lb;  // (read only where d >= 0)
  const uint32_t whole = la > ext ? la : ext;
  const uint32_t len = rec.d >= 0 ? whole : rec.ov;
  return rec.n ? len : 0u;
}

// ---- which reads cover column p, and where ----
struct MrgSources {
  bool in_a, in_b;
  uint32_t i, j;  // rows of a and of b; each means something only where its read covers p
};
SASSY_HAM_HD MrgSources mrg_sources(uint32_t p, uint32_t la, uint32_t lb, int32_t d) {
  const int32_t j = (int32_t)p - d;
  const bool in_b = (j >= 0) & (j < (int32_t)lb);  // (& for &&: no branch)
  return MrgSources{p < la, in_b, p, (uint32_t)j};
}

// ---- the consensus of one column, on bytes and integers ----
struct MrgByte {
  uint32_t c, q;
};
// Both reads cover the column.  Equal bytes: that byte, the higher quality.  Different bytes (as bytes: the profile's relation
// is not asked): the byte of the higher quality, a's on a tie, with quality min(126, 33 + max(2, |qa - qb|)) -- FLASH's rule
// with the tie fixed.  (Selects on scalars, no branch: the kernel calls this 64 times a lane.)
SASSY_HAM_HD MrgByte mrg_consensus(uint32_t ca, uint32_t qa, uint32_t cb, uint32_t qb) {
  const bool equal = ca == cb, a_wins = qa >= qb;
  const uint32_t hi = a_wins ? qa : qb, lo = a_wins ? qb : qa;
  const uint32_t diff = hi - lo, least = diff > 2u ? diff : 2u;
  const uint32_t raised = 33u + least, capped = raised < 126u ? raised : 126u;
  return MrgByte{a_wins ? ca : cb, equal ? hi : capped};
}
// One column out of what covers it; a column that nothing covers (there is none below the merged length) is zero.
SASSY_HAM_HD MrgByte mrg_column(bool in_a, bool in_b, uint32_t ca, uint32_t qa, uint32_t cb, uint32_t qb) {
  const MrgByte both = mrg_consensus(ca, qa, cb, qb);
  const uint32_t c = (in_a & in_b) ? both.c : in_a ? ca : in_b ? cb : 0u;
  const uint32_t q = (in_a & in_b) ? both.q : in_a ? qa : in_b ? qb : 0u;
  return MrgByte{c, q};
}

// ---- four columns at once: one 32-bit word of the merged text and of the merged quality ----
// Columns p0 .. p0 + 3 (p0 a multiple of 4), byte t of a word = column p0 + t.  wa / wqa: a's bytes and qualities at rows
// p0 .. p0 + 3 (what lies behind la is not looked at).  wb / wqb: R2's bytes and qualities, NOT yet complemented, already
// in b's order: byte t = row p0 + t - d of b (what lies outside of 0 .. lb is not looked at).  Columns at or behind len
// are zero in both words.
struct MrgWord {
  uint32_t text, qual;
};
SASSY_HAM_HD MrgWord mrg_word(uint32_t profile, uint32_t p0, uint32_t la, uint32_t lb, int32_t d, uint32_t len, uint32_t wa, uint32_t wqa,
                              uint32_t wb, uint32_t wqb) {
  MrgWord out{0u, 0u};
#pragma unroll
  for (uint32_t t = 0; t < 4; ++t) {
    const uint32_t p = p0 + t;
    const MrgSources s = mrg_sources(p, la, lb, d);
    const uint32_t cb = ovl_complement(profile, (wb >> (8u * t)) & 255u);
    const MrgByte col = mrg_column(s.in_a, s.in_b, (wa >> (8u * t)) & 255u, (wqa >> (8u * t)) & 255u, cb, (wqb >> (8u * t)) & 255u);
    const bool live = p < len;
    out.text |= (live ? col.c : 0u) << (8u * t);
    out.qual |= (live ? col.q : 0u) << (8u * t);
  }
  return out;
}

// ---- where block `pb` (columns pb .. pb + 63 of a merged read, pb a multiple of 64) finds R2's bytes ----
// Column p is row j = p - d of b, which is byte lb - 1 - j of R2: the block's 64 columns are the R2 bytes
// first .. first + 63 in descending order, first = lb - 64 + d - pb (negative where the block reaches beyond R2's head).
SASSY_HAM_HD int64_t mrg_r2_first(uint32_t pb, uint32_t lb, int32_t d) { return (int64_t)lb - 64 + (int64_t)d - (int64_t)pb; }
// word j of the block in b's order out of the sixteen words w[0 .. 16) that hold R2's bytes first .. first + 63 ascending
SASSY_HAM_HD uint32_t mrg_reverse_word(uint32_t w) { return (w >> 24) | ((w >> 8) & 0xFF00u) | ((w << 8) & 0xFF0000u) | (w << 24); }

}  // namespace sassy_hip
