// demux_step_driver.cc -- demux_step.h as the kernels of demux_reads.hip call it, on the host, against a byte-wise brute force.
// A stand-alone program with its own main and no HIP: tests/test_demux_reads_cpu.py builds it with the host compiler under
// AddressSanitizer and UBSan and runs it.  A lane of demux_assign_kernel is simulated word for word -- the window through
// trm_window_block out of a text whose pads hold garbage, the planes, the loop over the barcodes with dmx_combine, the
// assignment, the record, the clip -- for every barcode length, window place, read length, end, profile and barcode count the
// kernels can meet; then the combine as a reduction in any order, the bounds, every refusal in its order, and the blocks of a
// gather as reads_window_write_kernel<.., GATHER> makes them.  Prints "ok" and what it counted; any difference ends it with 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sassy_amd/csrc/demux_step.h"

using namespace sassy_hip;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
static uint32_t rnd_below(uint32_t n) { return rnd() % n; }

[[noreturn]] static void die(const char* what, long a = 0, long b = 0, long c = 0) {
  std::printf("FAILED %s (%ld %ld %ld)\n", what, a, b, c);
  std::exit(1);
}
#define CHECK(cond, ...) \
  do {                   \
    if (!(cond)) die(#cond, ##__VA_ARGS__); \
  } while (0)

static const char* kDnaLetters = "ACGT";
static const char* kIupacLetters = "ACGTNRYKMSWBDHVacgtnX-U";
static uint8_t letter(uint32_t profile) {
  return profile == kHamDna ? (uint8_t)kDnaLetters[rnd_below(4)] : (uint8_t)kIupacLetters[rnd_below((uint32_t)std::strlen(kIupacLetters))];
}

struct Text {
  std::vector<uint8_t> bytes;  // a multiple of 64
  std::vector<uint64_t> start, len;
};
// the reads at multiples of 64 with GARBAGE in every pad: what is read past a read's end must not show
static Text lay_out(const std::vector<std::vector<uint8_t>>& reads) {
  Text t;
  uint64_t at = 0;
  for (const auto& r : reads) {
    t.start.push_back(at);
    t.len.push_back(r.size());
    at += fq_round64(r.size());
  }
  t.bytes.resize(at);
  for (auto& b : t.bytes) b = (uint8_t)(0x80u | rnd_below(128));
  for (size_t i = 0; i < reads.size(); ++i)
    if (!reads[i].empty()) std::memcpy(t.bytes.data() + t.start[i], reads[i].data(), reads[i].size());
  return t;
}

struct Loader {
  const uint8_t* base;
  uint64_t bytes;
  void operator()(uint64_t at, uint32_t* w) const {
    CHECK(at % 16 == 0 && at + 16 <= bytes, (long)at, (long)bytes);
    std::memcpy(w, base + at, 16);
  }
};

struct Lane {
  DmxRecord rec;
  uint32_t label;
  DmxClip clip;
};
// one lane of demux_assign_kernel, and what demux_place_kernel derives from its record
template <int P, bool IUPAC>
static Lane lane(const Text& t, uint64_t read, const std::vector<uint32_t>& tab, uint32_t B, uint32_t m, uint32_t at, bool end3, uint32_t k,
                 uint32_t min_delta, bool keep_barcode) {
  constexpr uint32_t profile = IUPAC ? kHamIupac : kHamDna;
  const uint64_t s0 = t.start[read], l = t.len[read], bytes = t.bytes.size();
  const bool fits = l <= kOvlMaxLen && s0 <= bytes && l <= bytes - s0;
  const uint32_t la = fits ? (uint32_t)l : 0u;
  const bool has_window = dmx_has_window(la, at, m);
  uint32_t blk[16];
  for (int j = 0; j < 16; ++j) blk[j] = 0u;
  if (has_window) trm_window_block(Loader{t.bytes.data(), bytes}, s0 + dmx_window(la, at, m, end3), bytes, m, blk);
  uint32_t rw[P + 1][2];
  dmx_planes<P>(profile, blk, rw);
  const uint32_t mask[2] = {dmx_row_mask(m, 0), dmx_row_mask(m, 1)};
  DmxBest best = dmx_none();
  for (uint32_t j = 0; j < B; ++j) best = dmx_combine(best, dmx_one(dmx_mismatches<P, IUPAC>(rw, tab.data() + (size_t)j * (2 * P), mask), j, m));
  const bool assigned = dmx_assigned(has_window, best, k, min_delta);
  Lane out;
  out.rec = dmx_record(has_window, assigned, best);
  out.label = dmx_label(assigned, best, B);
  CHECK(dmx_record_label(out.rec, B) == out.label);
  const bool again = out.rec.sample != 0xFFFFFFFFu && dmx_has_window(la, at, m);  // (the place kernel reads it back)
  CHECK(again == assigned);
  out.clip = dmx_clip(la, at, m, end3, keep_barcode, again);
  return out;
}

struct Counts {
  long cases = 0, assigned = 0, ties = 0, no_window = 0, refusals = 0, blocks = 0, reductions = 0;
};

static void walk_cases(uint32_t profile, Counts& n) {
  const uint32_t ms[] = {1, 8, 31, 32, 33, 63, 64}, Bs[] = {1, 2, 63, 64, 65};
  std::vector<uint32_t> ats;
  for (uint32_t a = 0; a < 16; ++a) ats.push_back(a);  // every residue mod 16
  for (uint32_t a : {63u, 64u, 127u, 128u, 447u, 448u}) ats.push_back(a);  // at and across the 64-byte boundaries
  const uint32_t P = ovl_planes(profile);
  for (uint32_t m : ms)
    for (uint32_t at : ats) {
      if (at + m > kOvlMaxLen) continue;
      for (int end3 = 0; end3 < 2; ++end3)
        for (uint32_t B : Bs) {
          // the barcodes: random, the second a neighbour of the first (ties and margins), one repeated
          std::vector<std::vector<uint8_t>> bcs(B, std::vector<uint8_t>(m));
          for (auto& b : bcs)
            for (auto& c : b) c = letter(profile);
          if (B >= 2) {
            bcs[1] = bcs[0];
            bcs[1][rnd_below(m)] = letter(profile);
          }
          if (B >= 63) bcs[B - 1] = bcs[B / 2];
          std::vector<uint32_t> tab((size_t)B * 2 * P);
          for (uint32_t j = 0; j < B; ++j) dmx_encode_barcode(profile, bcs[j].data(), m, tab.data() + (size_t)j * 2 * P);
          const uint32_t las[] = {at + m - 1, at + m, at + m + 1, 0u, kOvlMaxLen};
          std::vector<std::vector<uint8_t>> reads;
          reads.push_back(std::vector<uint8_t>(1 + rnd_below(100), (uint8_t)'A'));  // (a read in front: s0 > 0)
          for (uint32_t la : las) {
            if (la > kOvlMaxLen) continue;
            std::vector<uint8_t> r(la);
            for (auto& c : r) c = letter(profile);
            if (la >= at + m && rnd_below(4)) {  // plant a barcode with up to two substitutions
              const uint32_t w = end3 ? la - at - m : at;
              std::memcpy(r.data() + w, bcs[rnd_below(B)].data(), m);
              for (uint32_t sub = rnd_below(3); sub; --sub) r[w + rnd_below(m)] = letter(profile);
            }
            reads.push_back(r);
          }
          const Text t = lay_out(reads);  // (the last read ends the text: a window's fifth piece may begin behind it)
          for (uint64_t read = 1; read < reads.size(); ++read) {
            static const uint32_t ks[] = {0, 1, 2, 64}, deltas[] = {0, 1, 2, 65};
            const uint32_t k = ks[rnd_below(4)], min_delta = deltas[rnd_below(4)];
            const bool keep = rnd_below(3) == 0;
            const Lane got = profile == kHamIupac ? lane<4, true>(t, read, tab, B, m, at, end3 != 0, k, min_delta, keep)
                                                  : lane<2, false>(t, read, tab, B, m, at, end3 != 0, k, min_delta, keep);
            // ---- byte by byte ----
            const std::vector<uint8_t>& a = reads[read];
            const uint32_t la = (uint32_t)a.size();
            const bool has = at + m <= la;
            uint32_t cost = 0xFFFFFFFFu, best = 0, second = m + 1, n_best = 0;
            std::vector<uint32_t> costs(B, 0);
            if (has) {
              const uint32_t w = end3 ? la - at - m : at;
              for (uint32_t j = 0; j < B; ++j)
                for (uint32_t i = 0; i < m; ++i) costs[j] += ham_match(profile, bcs[j][i], a[w + i]) ? 0u : 1u;
              for (uint32_t j = 0; j < B; ++j)
                if (costs[j] < cost) {
                  cost = costs[j];
                  best = j;
                }
              for (uint32_t j = 0; j < B; ++j) {
                n_best += costs[j] == cost;
                if (j != best) second = std::min(second, costs[j]);
              }
            }
            const bool assigned = has && cost <= k && second - cost >= min_delta;
            CHECK(got.rec.sample == (assigned ? best : 0xFFFFFFFFu), m, at, la);
            CHECK(got.rec.best == (has ? best : 0xFFFFFFFFu), m, at, la);
            CHECK(got.rec.tail == (has ? (cost | (second << 8) | (n_best << 16)) : 0x0000FFFFu), m, at, la);
            CHECK(got.label == (assigned ? best : B), m, at, la);
            const bool clip = assigned && !keep;
            const uint32_t lo = clip && !end3 ? at + m : 0u, hi = clip && end3 ? la - at - m : la;
            CHECK(got.clip.begin == lo && got.clip.len == hi - lo, m, at, la);
            CHECK((uint64_t)got.clip.begin + got.clip.len <= la, m, at, la);
            n.cases++;
            n.assigned += assigned;
            n.ties += has && n_best > 1;
            n.no_window += !has;
          }
        }
    }
}

// the combine as a reduction: any split of a set of (cost, index) gives what the walk in order gives
static void walk_reductions(Counts& n) {
  for (int round = 0; round < 2000; ++round) {
    const uint32_t B = 1 + rnd_below(70), m = 1 + rnd_below(64);
    std::vector<uint32_t> cost(B), idx(B);
    for (uint32_t j = 0; j < B; ++j) {
      cost[j] = rnd_below(std::min(m, 3u) + 1);
      idx[j] = j;
    }
    DmxBest seq = dmx_none();
    for (uint32_t j = 0; j < B; ++j) seq = dmx_combine(seq, dmx_one(cost[j], j, m));
    for (uint32_t i = B; i > 1; --i) std::swap(idx[i - 1], idx[rnd_below(i)]);
    const uint32_t cut = rnd_below(B + 1);
    DmxBest x = dmx_none(), y = dmx_none();
    for (uint32_t i = 0; i < cut; ++i) x = dmx_combine(dmx_one(cost[idx[i]], idx[i], m), x);
    for (uint32_t i = cut; i < B; ++i) y = dmx_combine(y, dmx_one(cost[idx[i]], idx[i], m));
    const DmxBest tree = rnd_below(2) ? dmx_combine(x, y) : dmx_combine(y, x);
    CHECK(tree.cost == seq.cost && tree.best == seq.best && tree.second == seq.second && tree.n == seq.n, round, B);
    CHECK(seq.second >= seq.cost && seq.n >= 1 && (B > 1 || seq.second == m + 1), round, B);
    n.reductions++;
  }
}

static void walk_bounds() {
  for (uint32_t B : {1u, 2u, 255u, 256u, 4095u, 4096u}) {
    const uint32_t bits = dmx_key_bits(B);
    CHECK(bits >= 1 && (B >> bits) == 0 && (bits == 1 || (B >> (bits - 1)) != 0), B, bits);
  }
  CHECK(dmx_key_bits(1) == 1 && dmx_key_bits(255) == 8 && dmx_key_bits(256) == 9 && dmx_key_bits(4096) == 13);
  for (int round = 0; round < 300; ++round) {
    const uint32_t B = 1 + rnd_below(9), n = rnd_below(40);
    std::vector<uint32_t> labels(n);
    for (auto& l : labels) l = rnd_below(3) ? rnd_below(B + 1) : B;
    std::sort(labels.begin(), labels.end());
    for (uint32_t s = 0; s <= B + 1; ++s) {
      const uint64_t got = dmx_lower_bound([&](uint64_t i) { return labels[i]; }, n, s);
      CHECK(got == (uint64_t)(std::lower_bound(labels.begin(), labels.end(), s) - labels.begin()), round, s);
    }
  }
}

static void walk_refusals(Counts& n) {
  const uint8_t bc0[] = "ACGT";
  const uint8_t* good[2] = {bc0, bc0};
  const uint8_t* holed[2] = {bc0, nullptr};
  DmxCall c{};  // everything wrong at once: each refusal hides the ones behind it
  c.have_searcher = false; c.flags = 4; c.min_delta = 66; c.n_barcodes = 0; c.barcode_len = 0; c.barcodes = nullptr; c.at = 600;
  ReadsGate& g = c.gate;
  g.handles = 1; g.profile = 0;
  g.overhang = g.only_best = g.max_n_frac = true; g.have_reads[0] = false; g.handle_read = false; g.device_s = 0; g.device_r[0] = 1; g.longest[0] = 513;
  c.have_bounds = c.have_sorted = false; g.in_flight = true;
  size_t which = 7;
  // (the call's own code, the gate's code, the barcode named)
  const auto expect = [&](DmxRefusal want, ReadsRefusal want_gate = kRdsOk, size_t want_which = 0) {
    ReadsRefusal gate = kRdsTooLong;
    const DmxRefusal got = dmx_refusal(c, &which, &gate);
    CHECK(got == want && gate == want_gate && which == want_which, (long)got, (long)gate, (long)which);
    n.refusals++;
  };
  expect(kDmxNullSearcher); c.have_searcher = true;
  expect(kDmxFlags); c.flags = kDmxEnd3 | kDmxKeepBarcode;
  expect(kDmxDelta); c.min_delta = 65;
  expect(kDmxCount); c.n_barcodes = 4097;
  expect(kDmxCount); c.n_barcodes = 2;
  expect(kDmxLen); c.barcode_len = 65;
  expect(kDmxLen); c.barcode_len = 4;
  expect(kDmxNullBarcode); c.barcodes = holed;
  expect(kDmxNullBarcode, kRdsOk, 1); c.barcodes = good;
  expect(kDmxAt); c.at = 509;
  expect(kDmxAt); c.at = 508;
  expect(kDmxGate, kRdsAscii); g.profile = kHamAsciiCi;
  expect(kDmxGate, kRdsAscii); g.profile = kHamIupac;
  expect(kDmxGate, kRdsOverhang); g.overhang = false;
  expect(kDmxGate, kRdsOnlyBest); g.only_best = false;
  expect(kDmxGate, kRdsNFrac); g.max_n_frac = false;
  expect(kDmxGate, kRdsNullReads); g.have_reads[0] = true;
  expect(kDmxNullOut);  // (the handle is not read yet: what it holds is judged late)
  g.handle_read = true;
  expect(kDmxGate, kRdsDevice); g.device_r[0] = 0;
  expect(kDmxGate, kRdsTooLong); g.longest[0] = 512;
  expect(kDmxNullOut); c.have_bounds = true;
  expect(kDmxNullOut); c.have_sorted = true;
  expect(kDmxGate, kRdsInFlight); g.in_flight = false;
  expect(kDmxOk);
  g.profile = kHamDna; c.flags = 0; c.min_delta = 0;
  expect(kDmxOk);
  CHECK(dmx_shifted(0) && !dmx_shifted(kDmxEnd3) && !dmx_shifted(kDmxKeepBarcode) && !dmx_shifted(kDmxEnd3 | kDmxKeepBarcode));
}

// the blocks of a gather: output record j is the window [begin, begin + len) of source read src[j], block by block as the
// write kernel makes them -- shifted through trm_window_block, or, where every begin is 0, through trm_aligned_quarter
static void walk_gather(Counts& n) {
  std::vector<std::vector<uint8_t>> reads;
  for (uint32_t la : {0u, 1u, 15u, 16u, 17u, 63u, 64u, 65u, 127u, 128u, 129u, 200u, 512u}) {
    std::vector<uint8_t> r(la);
    for (auto& c : r) c = (uint8_t)(33 + rnd_below(90));
    reads.push_back(r);
  }
  const Text t = lay_out(reads);
  const Loader load{t.bytes.data(), t.bytes.size()};
  for (int round = 0; round < 400; ++round) {
    const uint64_t from = rnd_below((uint32_t)reads.size());  // (repeats, skips, any order)
    const uint32_t la = (uint32_t)reads[from].size();
    for (uint32_t begin = 0; begin <= std::min(la, 17u); ++begin) {  // every residue mod 16
      for (int aligned = 0; aligned < 2; ++aligned) {
        if (aligned && begin) continue;
        const uint32_t len = rnd_below(2) ? la - begin : rnd_below(la - begin + 1);
        for (uint32_t b = 0; b * 64 < len; ++b) {
          const uint32_t left = len - 64 * b, keep = std::min(left, 64u);
          const uint64_t src = t.start[from] + begin + 64ull * b;
          uint32_t out[16];
          if (aligned) {
            for (uint32_t q = 0; q < 4; ++q) {
              uint32_t w[4];
              trm_aligned_quarter(load, src, t.bytes.size(), keep, q, w);
              std::memcpy(out + 4 * q, w, 16);
            }
          } else {
            trm_window_block(load, src, t.bytes.size(), keep, out);
          }
          uint8_t want[64];
          std::memset(want, 0, 64);
          std::memcpy(want, reads[from].data() + begin + 64 * b, keep);
          CHECK(std::memcmp(out, want, 64) == 0, (long)from, begin, b);
          n.blocks++;
        }
      }
    }
  }
}

int main() {
  Counts n;
  walk_cases(kHamDna, n);
  walk_cases(kHamIupac, n);
  walk_reductions(n);
  walk_bounds();
  walk_refusals(n);
  walk_gather(n);
  CHECK(n.assigned > n.cases / 10 && n.ties > n.cases / 50 && n.no_window > n.cases / 10, n.assigned, n.ties, n.no_window);
  std::printf("ok cases=%ld assigned=%ld ties=%ld no_window=%ld reductions=%ld refusals=%ld blocks=%ld\n", n.cases, n.assigned, n.ties, n.no_window,
              n.reductions, n.refusals, n.blocks);
  return 0;
}
