// hamming_plan.h -- what the host decides for the Hamming family (hamming.hip, amplicons.hip) before and between its launches,
// free of HIP: pure functions over plain structs, driven on the CPU by tests/c/hamming_plan_driver.cc.  In the order of a call:
// the patterns as scanned, the launch groups, a group's tables and launch shape, the step after a launch whose items
// overflowed the list, the text batches of the _many calls, the copies of a counts table, the popcount prefix of the items.
// A profile is named by value (hamming_step.h: kHamDna, kHamIupac, kHamAsciiCi, anything else plain Ascii).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "hamming_step.h"

namespace sassy_hip {

constexpr uint32_t kHamSlots = 64;                        // profile slots of a launch (= kMaxSlots, common.h)
constexpr uint32_t kHamStageBytes = kHamTileBlocks * 64;  // a tile's text
constexpr uint32_t kHamLdsBudget = 160 * 1024;
// LDS of one wavefront: the staged tile, then (slots + 1) rows of nb masks -- the last row is the N mask --, whole 16 bytes
constexpr uint32_t ham_lds_per_wave(uint32_t slots, uint32_t nb) { return (kHamStageBytes + (slots + 1) * nb * 8u + 15u) & ~15u; }

// One item: the hits of one pattern in one block.  Laid out as a Candidate so that sort_kernels.hip sorts it by `key`.
struct HamItem {
  uint64_t key;   // launch-local pattern index (pattern and strand) << 32 | block
  uint64_t mask;  // bit i: start 64 block + i is a hit
};
// per pattern of a launch, kHamTabWords words: rows, offset of its row slots (words) in `rows`, offset of its bytes in `pats`,
// N threshold (kHamNoFilter: none), pattern index of the call, strand
constexpr uint32_t kHamTabWords = 8;
constexpr uint32_t kHamNoFilter = 0xFFFFFFFFu;

constexpr bool ham_is_ascii(uint32_t profile) { return profile != kHamDna && profile != kHamIupac; }
inline uint32_t ham_slot_key(uint32_t profile, uint8_t c) {  // what a pattern byte's slot is keyed by
  if (profile == kHamDna) return (c >> 1) & 3u;
  if (profile == kHamIupac) return ham_iupac_nib(c);
  return profile == kHamAsciiCi ? ham_fold(c) : c;
}

// ---- the patterns as scanned ----
// One pattern of the call on one strand, as it is scanned.
struct HamPattern {
  uint32_t idx, strand;
  std::vector<uint8_t> bytes;  // strand 1: the reverse complement
  uint32_t nmax;               // most N a hit's span may hold (kHamNoFilter: no filter)
};
// Pattern `idx` on the + strand and -- rc -- its reverse complement on the - strand behind it, both with the N threshold of
// max_n_frac (NaN: none).  Nothing is added, and false returned, where the pattern can have no hit: not even a span without
// N passes, or no text is as long as the pattern.  complement(byte) is the profile's (profiles.h: complement_char).
template <typename Complement>
inline bool ham_add_scanned(uint32_t idx, const uint8_t* p, size_t m, bool rc, float max_n_frac, uint64_t longest_text,
                            const Complement& complement, std::vector<HamPattern>& out) {
  uint32_t nmax = kHamNoFilter;
  if (!std::isnan(max_n_frac)) {
    const int64_t c = ham_n_max((uint32_t)m, max_n_frac);
    if (c < 0) return false;
    if (c < (int64_t)m) nmax = (uint32_t)c;
  }
  if (longest_text < m) return false;
  out.push_back(HamPattern{idx, 0, std::vector<uint8_t>(p, p + m), nmax});
  if (rc) {
    HamPattern minus{idx, 1, {}, nmax};
    for (size_t j = m; j-- > 0;) minus.bytes.push_back(complement(p[j]));
    out.push_back(std::move(minus));
  }
  return true;
}
// A call's patterns in the contract's order: pattern, then + before -.
template <typename Complement>
inline std::vector<HamPattern> ham_scanned_patterns(const uint8_t* const* patterns, const size_t* lens, size_t n, bool rc, float max_n_frac,
                                                    uint64_t longest_text, const Complement& complement) {
  std::vector<HamPattern> all;
  for (size_t i = 0; i < n; ++i) ham_add_scanned((uint32_t)i, patterns[i], lens[i], rc, max_n_frac, longest_text, complement, all);
  return all;
}

// ---- launch groups ----
// Patterns [a0, a1) of the scanned list share a launch and its slots.
struct HamGroup {
  size_t a0 = 0, a1 = 0;
  uint32_t ns = 0;               // slots in use: Dna 4, Iupac 16, Ascii one per distinct (folded) byte of the group
  int slot_of[256];              // slot of a pattern byte's key (ham_slot_key), -1: none
  uint8_t slot_val[kHamSlots] = {};  // per slot what it tests (ScanParams::slot_val)
};
inline size_t ham_batch_patterns(long hamming_batch) { return hamming_batch > 0 ? (size_t)hamming_batch : 512; }
// The group that starts at a0, greedy: at most `max_batch` patterns, and for Ascii as many as share kHamSlots slots (a
// pattern alone always fits: the entry points refuse more distinct bytes).
inline HamGroup ham_next_group(uint32_t profile, const std::vector<HamPattern>& all, size_t a0, size_t max_batch) {
  HamGroup G;
  G.ns = profile == kHamDna ? 4u : profile == kHamIupac ? 16u : 0u;
  if (profile == kHamIupac)
    for (uint32_t s = 0; s < 16; ++s) G.slot_val[s] = (uint8_t)s;  // a slot per base set
  std::fill(G.slot_of, G.slot_of + 256, -1);
  const bool ascii = ham_is_ascii(profile);
  if (!ascii)
    for (uint32_t s = 0; s < G.ns; ++s) G.slot_of[s] = (int)s;
  for (G.a0 = G.a1 = a0; G.a1 < all.size() && G.a1 - a0 < max_batch; ++G.a1) {
    if (!ascii) continue;
    HamGroup with = G;  // the group with this pattern's bytes: taken if they still share the slots
    for (uint8_t c : all[G.a1].bytes) {
      const uint32_t key = ham_slot_key(profile, c);
      if (with.slot_of[key] < 0 && with.ns < kHamSlots) { with.slot_of[key] = (int)with.ns; with.slot_val[with.ns++] = (uint8_t)key; }
      else if (with.slot_of[key] < 0) return G;
    }
    G = with;
  }
  return G;
}
// Amplicons: a pair's 2 `sides` scanned patterns never straddle two groups, so a group takes whole pairs.
inline size_t ham_group_pairs(size_t max_batch, uint32_t sides) { return std::max<size_t>(1, max_batch / (2 * sides)); }

// ---- a group's tables, launch shape and list sizes ----
struct HamTables {
  // tab: kHamTabWords words per pattern; rows: every pattern's row slots, a byte each, four to a word; pats: the patterns as
  // scanned, one behind the other
  std::vector<uint32_t> tab, rows;
  std::vector<uint8_t> pats;
  uint32_t longest = 0, halo = 0, nb = 0;  // the longest pattern, its halo blocks, 64 + halo
  bool n_filter = false;                   // some pattern has an N threshold
  uint32_t ns_t = 0, wpg = 0;              // slots of the kernel instantiation: 4, 16 or 64; wavefronts per workgroup, 1 .. 4
  size_t smem = 0;                         // wpg wavefronts' LDS, within the budget
  // the item list's first size and the size it may grow to; tiles of one launch: its item counter cannot wrap
  uint64_t item_cap = 0, max_cap = 0, span_max = 0;
};
inline HamTables ham_tables(uint32_t profile, const HamPattern* pats, uint32_t np, const HamGroup& G, long hamming_items) {
  HamTables T;
  T.tab.assign((size_t)np * kHamTabWords, 0u);
  for (uint32_t p = 0; p < np; ++p) {
    const HamPattern& hp = pats[p];
    const uint32_t m = (uint32_t)hp.bytes.size();
    T.longest = std::max(T.longest, m);
    uint32_t* row = &T.tab[(size_t)p * kHamTabWords];
    row[0] = m; row[1] = (uint32_t)T.rows.size(); row[2] = (uint32_t)T.pats.size(); row[3] = hp.nmax; row[4] = hp.idx; row[5] = hp.strand;
    T.n_filter = T.n_filter || hp.nmax != kHamNoFilter;
    T.rows.resize(T.rows.size() + (m + 3) / 4, 0u);
    for (uint32_t j = 0; j < m; ++j) T.rows[row[1] + (j >> 2)] |= (uint32_t)G.slot_of[ham_slot_key(profile, hp.bytes[j])] << (8 * (j & 3));
    T.pats.insert(T.pats.end(), hp.bytes.begin(), hp.bytes.end());
  }
  T.halo = ham_halo_blocks(T.longest);
  T.nb = kHamTileBlocks + T.halo;
  T.ns_t = profile == kHamDna ? 4u : (profile == kHamIupac || G.ns <= 16) ? 16u : 64u;
  const uint32_t per_wave = ham_lds_per_wave(T.ns_t, T.nb);
  T.wpg = std::min<uint32_t>(4, kHamLdsBudget / per_wave);
  T.smem = (size_t)T.wpg * per_wave;
  const uint64_t min_cap = (uint64_t)np * kHamTileBlocks;  // one tile always fits
  T.item_cap = std::max<uint64_t>(hamming_items > 0 ? (uint64_t)hamming_items : (1u << 16), min_cap);
  T.max_cap = hamming_items > 0 ? T.item_cap : std::max<uint64_t>(min_cap, 1u << 22);
  T.span_max = std::max<uint64_t>(1, (0x7FFFFFFFull / kHamTileBlocks) / np);
  return T;
}

// ---- after a launch over `span` tiles that counted `count` items for a list of item_cap ----
struct HamStep {
  enum What { Done, Again, Overflow } what;  // the items are all there | launch again | min_span tiles do not fit max_cap items
  uint64_t item_cap, span;                   // for the next launch (Overflow: the list as it was grown)
};
// Nothing of an overflowing launch is used: first a larger list (count and a quarter, at most max_cap), then a shorter range
// in proportion, never below min_span (with min_span == 1 never Overflow: one tile always fits).
inline HamStep ham_overflow_step(uint64_t count, uint64_t item_cap, uint64_t max_cap, uint64_t span, uint64_t min_span) {
  if (count <= item_cap) return {HamStep::Done, item_cap, span};
  if (item_cap < max_cap && count <= max_cap) item_cap = std::min<uint64_t>(max_cap, count + count / 4);
  else if (item_cap < max_cap) item_cap = max_cap;
  if (count > item_cap) {
    if (span <= min_span) return {HamStep::Overflow, item_cap, span};
    span = std::max<uint64_t>(min_span, std::min<uint64_t>(span - 1, span * item_cap / count));
  }
  return {HamStep::Again, item_cap, span};
}

// ---- the text batches of the _many calls ----
// Texts [t0, t1) laid out in one buffer of `total` bytes, each from a multiple of 64 bytes on; an empty text takes no block.
struct HamTextBatch {
  size_t t0 = 0, t1 = 0;
  uint64_t total = 0, longest = 0;
  std::vector<uint64_t> start, len;
};
inline uint64_t ham_many_batch_bytes(long hamming_many_batch) { return hamming_many_batch > 0 ? (uint64_t)hamming_many_batch : (1ull << 30); }
// The batch that starts at text t0: as many texts as stay within batch_cap bytes, a longer text alone.
inline HamTextBatch ham_next_text_batch(const size_t* text_lens, size_t n_texts, size_t t0, uint64_t batch_cap) {
  HamTextBatch B;
  B.t0 = B.t1 = t0;
  while (B.t1 < n_texts) {
    const uint64_t slot = ((uint64_t)text_lens[B.t1] + 63) / 64 * 64;
    if (B.t1 > t0 && B.total + slot > batch_cap) break;
    B.start.push_back(B.total);
    B.len.push_back(text_lens[B.t1]);
    B.longest = std::max<uint64_t>(B.longest, text_lens[B.t1]);
    B.total += slot;
    ++B.t1;
  }
  return B;
}

// Copies of a counts table of n_bins counters (a power of two).  In the worst case -- every wavefront holds hits of one cost of
// one pattern -- every tile adds to one word, and a launch of few patterns streams tiles at the rate of HBM: 6.3 TB/s over 4 KiB
// tiles is about 1 500 adds per microsecond where one contended word takes about 88: 18 words are needed, 32
// are kept while 32 tables stay within 2^16 counters (512 KiB to clear and to read back), fewer for a larger table -- whose
// launches hold more patterns per tile and so add to one word less often --, one at least.  `forced` > 0: that many (option
// hamming_count_copies; rounded down to a power of two, at most 1024, within 2^26 counters).
inline uint32_t hamming_count_copies(uint64_t n_bins, long forced) {
  uint32_t copies = 32;
  uint64_t room = 1ull << 16;
  if (forced > 0) {
    copies = 1;
    while (copies * 2 <= (uint64_t)std::min<long>(forced, 1024)) copies *= 2;
    room = 1ull << 26;
  }
  while (copies > 1 && (uint64_t)copies * n_bins > room) copies /= 2;
  return copies;
}

// The popcount prefix of a range's sorted items: prefix[i] = hits of the items in front of item i, prefix[n] = *hits, all of
// them.  False: the range's hits, or with them the `already` records of the call, do not fit 32 bits.
inline bool ham_prefix(const std::vector<HamItem>& items, uint64_t already, std::vector<uint32_t>& prefix, uint64_t* hits) {
  prefix.resize(items.size() + 1);
  uint64_t h = 0;
  for (size_t i = 0; i < items.size(); ++i) {
    prefix[i] = (uint32_t)h;
    h += (uint64_t)__builtin_popcountll(items[i].mask);
  }
  prefix[items.size()] = (uint32_t)h;
  *hits = h;
  return h <= 0xFFFFFFFFull && already + h <= 0xFFFFFFFFull;
}

}  // namespace sassy_hip
