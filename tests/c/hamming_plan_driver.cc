// hamming_plan_driver.cc -- drives sassy_amd/csrc/hamming_plan.h (what the host decides for the Hamming family, free of HIP)
// on the host: the scanned patterns against an independent restatement, the launch groups' invariants, a group's tables
// decoded again, the overflow step on the cases read off the driver and on random chains, the text batches, the copies of a
// counts table, the popcount prefix.  Built by tests/test_hamming_plan_cpu.py with -fsanitize=address,undefined.
//   hamming_plan_driver <seed>   prints "ok patterns=<n> groups=<n> tables=<n> chains=<n> batches=<n>", exit status 0;
//                                a failed check: its line on stderr, 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <bitset>
#include <string>
#include <vector>

#include "../../sassy_amd/csrc/hamming_plan.h"

using namespace sassy_hip;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

constexpr uint32_t kAscii = 0;
static const char kIupacFrom[] = "ACTGRYSWKMBDHVNX", kIupacTo[] = "TGACYRSWMKVHDBNX";

// the profiles' complement, restated: Dna upper-case ACGT only, Iupac every letter in both cases
static uint8_t complement(uint32_t profile, uint8_t c) {
  const char* at = c ? strchr(kIupacFrom, c & ~0x20) : nullptr;
  if (!at || (profile == kHamDna && ((c & 0x20) || at - kIupacFrom >= 4))) return c;
  return (uint8_t)(kIupacTo[at - kIupacFrom] | (c & 0x20));
}
// the slot key, restated from the profiles' definitions
static uint32_t key_of(uint32_t profile, uint8_t c) {
  if (profile == kHamDna) return (c >> 1) & 3u;
  if (profile == kHamIupac) {
    static const char* sets[16] = {"X", "A", "C", "M", "TU", "W", "Y", "H", "G", "R", "S", "V", "K", "D", "B", "N"};
    for (uint32_t s = 0; s < 16; ++s)
      if (strchr(sets[s], c & ~0x20) && c >= 'A') return s;
    return 15;
  }
  return profile == kHamAsciiCi && c >= 'A' && c <= 'Z' ? c + 32u : c;
}
static std::vector<uint8_t> random_pattern(uint32_t profile, size_t m, uint32_t base = 0, uint32_t width = 0) {
  std::vector<uint8_t> p(m);
  for (uint8_t& c : p)
    c = profile == kHamDna ? "ACGTacgtN"[below(9)] : profile == kHamIupac ? "ACGTURYSWKMBDHVNXacgtn"[below(22)] : (uint8_t)(base + below(width));
  return p;
}

static uint64_t n_patterns_checked, n_groups, n_tables, n_chains, n_batches;

static void scanned_patterns() {
  const float fracs[] = {NAN, 0.0f, 0.1f, 1.0f, -0.5f};
  for (uint32_t profile : {kHamDna, kHamIupac, kAscii})
    for (int rc = 0; rc < (profile == kAscii ? 1 : 2); ++rc)
      for (float frac : fracs)
        for (int rep = 0; rep < 40; ++rep) {
          const size_t n = 1 + below(12);
          const uint64_t longest_text = 1 + below(48);
          std::vector<std::vector<uint8_t>> pats;
          std::vector<const uint8_t*> ptr;
          std::vector<size_t> lens;
          for (size_t i = 0; i < n; ++i) pats.push_back(random_pattern(profile, 1 + below(56), 32, 90));
          for (const auto& p : pats) { ptr.push_back(p.data()); lens.push_back(p.size()); }
          const std::vector<HamPattern> got =
              ham_scanned_patterns(ptr.data(), lens.data(), n, rc != 0, frac, longest_text, [&](uint8_t c) { return complement(profile, c); });
          size_t at = 0;
          for (size_t i = 0; i < n; ++i) {
            const size_t m = lens[i];
            // the threshold: the largest count whose fraction of m passes, no filter where that is m itself
            long best = -1;
            for (long c = (long)m; c >= 0 && best < 0; --c)
              if ((float)c / (float)m <= frac) best = c;
            if (!std::isnan(frac) && best < 0) continue;  // no hit can pass
            if (m > longest_text) continue;               // no text holds it
            const uint32_t nmax = std::isnan(frac) || best == (long)m ? kHamNoFilter : (uint32_t)best;
            for (uint32_t strand = 0; strand < (rc ? 2u : 1u); ++strand, ++at) {
              CHECK(at < got.size());
              const HamPattern& g = got[at];
              CHECK(g.idx == i && g.strand == strand && g.nmax == nmax && g.bytes.size() == m);
              for (size_t j = 0; j < m; ++j) CHECK(g.bytes[j] == (strand ? complement(profile, pats[i][m - 1 - j]) : pats[i][j]));
            }
          }
          CHECK(at == got.size());
          n_patterns_checked += got.size();
        }
}

static std::bitset<256> keys_of(uint32_t profile, const std::vector<HamPattern>& all, size_t a0, size_t a1) {
  std::bitset<256> keys;
  for (size_t a = a0; a < a1; ++a)
    for (uint8_t c : all[a].bytes) keys.set(key_of(profile, c));
  return keys;
}
static void check_groups(uint32_t profile, const std::vector<HamPattern>& all, long batch_sw, bool one_each) {
  const size_t max_batch = ham_batch_patterns(batch_sw);
  CHECK(max_batch == (batch_sw > 0 ? (size_t)batch_sw : 512));
  size_t a0 = 0;
  while (a0 < all.size()) {
    const HamGroup G = ham_next_group(profile, all, a0, max_batch);
    CHECK(G.a0 == a0 && G.a1 > a0 && G.a1 <= all.size() && G.a1 - a0 <= max_batch);  // in order, none left out, none twice
    if (ham_is_ascii(profile)) {
      const std::bitset<256> keys = keys_of(profile, all, G.a0, G.a1);
      CHECK(keys.count() <= 64 && G.ns == keys.count());
      for (uint32_t key = 0; key < 256; ++key) {
        CHECK((G.slot_of[key] >= 0) == keys.test(key));
        if (G.slot_of[key] >= 0) CHECK((uint32_t)G.slot_of[key] < G.ns && G.slot_val[G.slot_of[key]] == key);
      }
      if (G.a1 < all.size() && G.a1 - a0 < max_batch) CHECK(keys_of(profile, all, G.a0, G.a1 + 1).count() > 64);  // maximal
      if (one_each) CHECK(G.a1 - a0 == 1);
    } else {
      CHECK(G.ns == (profile == kHamDna ? 4u : 16u));
      CHECK(G.a1 - a0 == std::min(max_batch, all.size() - a0));  // maximal
      for (uint32_t key = 0; key < 256; ++key) CHECK(G.slot_of[key] == (key < G.ns ? (int)key : -1));
      if (profile == kHamIupac)
        for (uint32_t s = 0; s < 16; ++s) CHECK(G.slot_val[s] == s);
    }
    a0 = G.a1;
    ++n_groups;
  }
}
static void groups() {
  for (uint32_t profile : {kHamDna, kAscii, kHamAsciiCi}) {
    std::vector<HamPattern> all;
    for (size_t n = 1; n <= 700; ++n) {
      // Ascii: every pattern from a window of 30 byte values, so that some neighbours share slots and some do not
      all.push_back(HamPattern{(uint32_t)n, 0, random_pattern(profile, 1 + below(16), 40 + (uint32_t)below(150), 30), kHamNoFilter});
      for (long batch_sw : {0L, 1L, 2L, 8L}) check_groups(profile, all, batch_sw, false);
    }
  }
  std::vector<HamPattern> disjoint;  // neighbours share no byte and 40 + 40 > 64: one pattern per group
  for (uint32_t i = 0; i < 30; ++i) {
    HamPattern p{i, 0, {}, kHamNoFilter};
    for (uint32_t j = 0; j < 40; ++j) p.bytes.push_back((uint8_t)(1 + 40 * (i % 6) + j));
    disjoint.push_back(p);
  }
  check_groups(kAscii, disjoint, 0, true);
  CHECK(ham_group_pairs(512, 2) == 128 && ham_group_pairs(512, 1) == 256 && ham_group_pairs(1, 2) == 1 && ham_group_pairs(8, 2) == 2);
}

static void tables() {
  for (uint32_t profile : {kHamDna, kHamIupac, kAscii, kHamAsciiCi})
    for (uint32_t m : {1u, 3u, 4u, 5u, 63u, 64u, 65u, 1024u})
      for (long items_sw : {0L, 1L, 64L, 300L}) {
        std::vector<HamPattern> all;
        const uint32_t np = 1 + (uint32_t)below(5);
        const uint32_t base = 40 + (uint32_t)below(100), width = 1 + (uint32_t)below(60);
        for (uint32_t p = 0; p < np; ++p)
          all.push_back(HamPattern{7 + p / 2, p & 1u, random_pattern(profile, p == np / 2 ? m : 1 + below(m), base, width),
                                   below(3) ? kHamNoFilter : (uint32_t)below(m)});
        const HamGroup G = ham_next_group(profile, all, 0, 512);
        CHECK(G.a0 == 0 && G.a1 == np);  // (at most 60 distinct bytes)
        const HamTables T = ham_tables(profile, all.data(), np, G, items_sw);
        CHECK(T.tab.size() == (size_t)np * kHamTabWords);
        size_t rows_at = 0, pats_at = 0;
        bool n_filter = false;
        for (uint32_t p = 0; p < np; ++p) {
          const uint32_t* row = &T.tab[(size_t)p * kHamTabWords];
          const HamPattern& hp = all[p];
          CHECK(row[0] == hp.bytes.size() && row[1] == rows_at && row[2] == pats_at && row[3] == hp.nmax && row[4] == hp.idx && row[5] == hp.strand);
          CHECK(row[6] == 0 && row[7] == 0);
          for (uint32_t j = 0; j < row[0]; ++j) {
            const uint32_t slot = (T.rows.at(row[1] + j / 4) >> (8 * (j % 4))) & 0xFFu, key = key_of(profile, hp.bytes[j]);
            CHECK(slot < G.ns && (profile == kHamDna ? slot : (uint32_t)G.slot_val[slot]) == key);
            CHECK(T.pats.at(row[2] + j) == hp.bytes[j]);
          }
          for (uint32_t j = row[0]; j < (row[0] + 3) / 4 * 4; ++j) CHECK(((T.rows.at(row[1] + j / 4) >> (8 * (j % 4))) & 0xFFu) == 0);
          rows_at += (row[0] + 3) / 4;
          pats_at += row[0];
          n_filter = n_filter || hp.nmax != kHamNoFilter;
        }
        CHECK(T.rows.size() == rows_at && T.pats.size() == pats_at && T.n_filter == n_filter);
        CHECK(T.longest == m && T.halo == (m - 1 + 63) / 64 && T.nb == 64 + T.halo);
        CHECK(T.ns_t == (profile == kHamDna ? 4u : profile == kHamIupac || G.ns <= 16 ? 16u : 64u) && T.ns_t >= G.ns);
        const uint32_t per_wave = ham_lds_per_wave(T.ns_t, T.nb);
        CHECK(per_wave % 16 == 0 && per_wave >= 4096 + (T.ns_t + 1) * T.nb * 8);
        CHECK(T.wpg >= 1 && T.wpg <= 4 && (size_t)T.wpg * per_wave <= 160 * 1024 && T.smem == (size_t)T.wpg * per_wave);
        CHECK(T.wpg == 4 || (size_t)(T.wpg + 1) * per_wave > 160 * 1024);
        const uint64_t one_tile = (uint64_t)np * 64;
        CHECK(T.item_cap >= one_tile && T.max_cap >= T.item_cap);
        if (items_sw > 0) CHECK(T.item_cap == std::max<uint64_t>((uint64_t)items_sw, one_tile) && T.max_cap == T.item_cap);
        else CHECK(T.item_cap == 65536 && T.max_cap == 4194304);
        CHECK(T.span_max >= 1 && T.span_max * one_tile <= 0x7FFFFFFFull && (T.span_max + 1) * one_tile > 0x7FFFFFFFull);
        ++n_tables;
      }
}

static void expect_step(uint64_t count, uint64_t item_cap, uint64_t max_cap, uint64_t span, uint64_t min_span, HamStep::What what,
                        uint64_t new_cap, uint64_t new_span) {
  const HamStep s = ham_overflow_step(count, item_cap, max_cap, span, min_span);
  CHECK(s.what == what && s.item_cap == new_cap && s.span == new_span);
}
static void overflow_step() {
  expect_step(65536, 65536, 4194304, 1000, 1, HamStep::Done, 65536, 1000);
  expect_step(100000, 65536, 4194304, 1000, 1, HamStep::Again, 125000, 1000);
  expect_step(5000000, 65536, 4194304, 1000, 1, HamStep::Again, 4194304, 838);
  expect_step(4000000, 65536, 4194304, 1000, 1, HamStep::Again, 4194304, 1000);
  expect_step(65, 64, 64, 1, 1, HamStep::Overflow, 64, 1);
  expect_step(600, 512, 512, 10, 3, HamStep::Again, 512, 8);
  expect_step(600, 512, 512, 3, 3, HamStep::Overflow, 512, 3);
  expect_step(5000, 512, 512, 10, 3, HamStep::Again, 512, 3);
  for (int rep = 0; rep < 20000; ++rep) {
    const bool forced = below(2) != 0;
    const uint64_t max_cap = forced ? 64 + below(5000) : 4194304;
    uint64_t item_cap = forced ? max_cap : 65536, min_span = 1 + below(5), span = min_span + below(1u << (1 + below(20)));
    const uint64_t per_tile = 1 + below(1u << (1 + below(14)));  // items a tile of this text holds, at most
    uint64_t last = ~0ull;
    int steps = 0;
    for (;; ++steps) {
      CHECK(steps < 64);
      const uint64_t count = std::min<uint64_t>(std::min(last, per_tile * span - below(per_tile)), 0xFFFFFFFFull);
      const HamStep s = ham_overflow_step(count, item_cap, max_cap, span, min_span);
      CHECK(s.span <= span && s.span >= min_span && s.item_cap >= item_cap && s.item_cap <= max_cap);
      if (s.what == HamStep::Done) { CHECK(count <= item_cap && s.span == span && s.item_cap == item_cap); break; }
      CHECK(count > item_cap);
      if (s.what == HamStep::Overflow) { CHECK(span <= min_span && count > max_cap && s.item_cap == max_cap); break; }
      CHECK(s.item_cap > item_cap || s.span < span);  // the next launch differs
      item_cap = s.item_cap; span = s.span; last = count;
    }
    ++n_chains;
  }
}

static void text_batches() {
  const size_t edge[] = {0, 1, 63, 64, 65};
  for (int rep = 0; rep < 400; ++rep) {
    const uint64_t cap = 4096 << below(3);
    std::vector<size_t> lens(1 + below(60));
    for (size_t& l : lens) l = below(3) ? edge[below(5)] : below(5000);
    lens[below(lens.size())] = cap + 1 + below(20000);  // a text longer than the cap
    size_t t0 = 0;
    while (t0 < lens.size()) {
      const HamTextBatch B = ham_next_text_batch(lens.data(), lens.size(), t0, cap);
      const size_t nt = B.t1 - B.t0;
      CHECK(B.t0 == t0 && nt >= 1 && B.t1 <= lens.size() && B.start.size() == nt && B.len.size() == nt);
      uint64_t at = 0, longest = 0;
      for (size_t i = 0; i < nt; ++i) {
        CHECK(B.start[i] == at && at % 64 == 0 && B.len[i] == lens[t0 + i]);  // (an empty text: the start of the text behind it)
        at += (lens[t0 + i] + 63) / 64 * 64;
        longest = std::max<uint64_t>(longest, lens[t0 + i]);
      }
      CHECK(B.total == at && B.longest == longest);
      CHECK(at <= cap || nt == 1);
      if (B.t1 < lens.size()) CHECK(at + (lens[B.t1] + 63) / 64 * 64 > cap);  // maximal
      t0 = B.t1;
      ++n_batches;
    }
  }
  CHECK(ham_many_batch_bytes(0) == (1ull << 30) && ham_many_batch_bytes(8192) == 8192);
}

static void count_copies_and_prefix() {
  CHECK(hamming_count_copies(2, 0) == 32 && hamming_count_copies(2048, 0) == 32 && hamming_count_copies(4096, 0) == 16);
  CHECK(hamming_count_copies(65536, 0) == 1 && hamming_count_copies(100000, 0) == 1);
  CHECK(hamming_count_copies(2, 5) == 4 && hamming_count_copies(2, 5000) == 1024 && hamming_count_copies(1ull << 20, 1024) == 64);
  for (int rep = 0; rep < 200; ++rep) {
    std::vector<HamItem> items(below(300));
    for (HamItem& it : items) it = HamItem{rnd(), below(4) ? rnd() & rnd() : ~0ull};
    std::vector<uint32_t> prefix;
    uint64_t hits = 0, want = 0;
    CHECK(ham_prefix(items, 0, prefix, &hits) && prefix.size() == items.size() + 1);
    for (size_t i = 0; i < items.size(); ++i) {
      CHECK(prefix[i] == want);
      for (uint64_t m = items[i].mask; m; m &= m - 1) ++want;
    }
    CHECK(prefix[items.size()] == want && hits == want);
    CHECK(ham_prefix(items, 0xFFFFFFFFull - want, prefix, &hits) && hits == want);
    CHECK(!ham_prefix(items, 0xFFFFFFFFull - want + 1, prefix, &hits) && hits == want);
  }
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  scanned_patterns();
  groups();
  tables();
  overflow_step();
  text_batches();
  count_copies_and_prefix();
  printf("ok patterns=%llu groups=%llu tables=%llu chains=%llu batches=%llu\n", (unsigned long long)n_patterns_checked,
         (unsigned long long)n_groups, (unsigned long long)n_tables, (unsigned long long)n_chains, (unsigned long long)n_batches);
  return 0;
}
