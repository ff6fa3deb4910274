// overlap_step_driver.cc -- drives sassy_amd/csrc/overlap_step.h (the arithmetic of sassy_hip_read_overlaps, free of HIP) on
// the host against a byte-wise brute force: the planes of both reads and the shifted-plane mismatch count at EVERY offset,
// for every length 0 .. 130, 191 .. 193, 511 and 512 on one side against the border lengths (and itself, and a random one)
// on the other, Dna and Iupac, at the word count the kernel would take and at the widest; the offset geometry and the range
// of offsets a call looks at; the acceptance test; the best offset and the accepted count as the kernel finds them (lanes
// as offsets, 64 per round, each lane its own best, a butterfly of ovl_combine) against one sequential walk of the rule as
// the definition states it; every refusal, in its order.  Built by tests/test_read_overlaps_cpu.py with
// -fsanitize=address,undefined.
//   overlap_step_driver <seed>        prints "ok pairs=<n> offsets=<n> bests=<n> refusals=<n>", exit status 0;
//                                     a failed check: its line on stderr, 1
//   overlap_step_driver complement    prints the 256 complements of each profile as hex, one line "dna <512 digits>", "iupac ..."
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sassy_amd/csrc/overlap_step.h"

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

static uint8_t random_byte(uint32_t profile, uint32_t flavour) {
  static const char iupac[] = "ACGTUNRYSWKMBDHVXacgtunry-";
  static const char dna[] = "ACGTacgt";
  if (flavour == 0) return (uint8_t)"ACGT"[below(4)];
  if (flavour == 1) return (uint8_t)"AAAC"[below(4)];  // low complexity: many accepted offsets
  if (profile == kHamIupac) return below(16) ? (uint8_t)iupac[below(sizeof(iupac) - 1)] : (uint8_t)below(256);
  return below(16) ? (uint8_t)dna[below(sizeof(dna) - 1)] : (uint8_t)below(256);
}

// ---- the definition, byte by byte ----
static uint32_t brute_mismatches(uint32_t profile, const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, int32_t d, uint32_t* ov_out) {
  const int32_t la = (int32_t)a.size(), lb = (int32_t)b.size();
  const int32_t lo = std::max(0, d), hi = std::min(la, d + lb);
  uint32_t mm = 0, ov = 0;
  for (int32_t i = lo; i < hi; ++i) {
    ++ov;
    mm += ham_match(profile, a[(size_t)i], b[(size_t)(i - d)]) ? 0u : 1u;
  }
  *ov_out = ov;
  return mm;
}
static std::vector<uint8_t> reverse_complement(uint32_t profile, const std::vector<uint8_t>& r2) {
  std::vector<uint8_t> b(r2.size());
  for (size_t t = 0; t < r2.size(); ++t) b[t] = (uint8_t)ovl_complement(profile, r2[r2.size() - 1 - t]);
  return b;
}

static uint32_t plane_mismatches(uint32_t profile, const uint32_t* a, const uint32_t* bpad, uint32_t W, int32_t d) {
  return profile == kHamIupac ? ovl_mismatches<4, true>(a, bpad, W, d) : ovl_mismatches<2, false>(a, bpad, W, d);
}

// the kernel's way to a pair's record: lanes as offsets, each lane its best over the rounds, then the butterfly
static OvlBest best_as_the_kernel(uint32_t profile, const uint32_t* a, const uint32_t* bpad, uint32_t W, uint32_t la, uint32_t lb, uint32_t min_overlap,
                                  uint32_t k, uint32_t permille) {
  const OvlRange range = ovl_offsets(la, lb, min_overlap);
  const int32_t d_last = range.d_first + (int32_t)range.count - 1;
  OvlBest lanes[kOvlWave];
  for (OvlBest& l : lanes) l = ovl_none();
  for (uint32_t round = 0; round < ovl_rounds(range.count); ++round)
    for (uint32_t lane = 0; lane < kOvlWave; ++lane) {
      const int32_t d_mine = range.d_first + (int32_t)(round * kOvlWave + lane);
      const bool in_range = d_mine <= d_last;
      const int32_t d = in_range ? d_mine : d_last;
      const uint32_t mm = plane_mismatches(profile, a, bpad, W, d), ov = ovl_overlap(la, lb, d);
      lanes[lane] = ovl_combine(lanes[lane], ovl_one(d, ov, mm, in_range && ovl_accepts(mm, ov, min_overlap, k, permille)));
    }
  for (uint32_t step = 32; step >= 1; step >>= 1) {
    OvlBest next[kOvlWave];
    for (uint32_t lane = 0; lane < kOvlWave; ++lane) next[lane] = ovl_combine(lanes[lane], lanes[lane ^ step]);
    memcpy(lanes, next, sizeof(lanes));
  }
  for (uint32_t lane = 1; lane < kOvlWave; ++lane)  // every lane ends with the same record
    CHECK(lanes[lane].d == lanes[0].d && lanes[lane].ov == lanes[0].ov && lanes[lane].mm == lanes[0].mm && lanes[lane].n == lanes[0].n);
  return lanes[0];
}
// the definition's: every offset of the pair, the rule as the issue states it, 64-bit products
// (mm_of[d + lb - 1], ov_of[d + lb - 1]: brute_mismatches of every offset, counted once per pair)
static OvlBest best_by_definition(int32_t la, int32_t lb, const std::vector<uint32_t>& mm_of, const std::vector<uint32_t>& ov_of, uint32_t min_overlap,
                                  uint32_t k, uint32_t permille) {
  OvlBest best = ovl_none();
  if (la == 0 || lb == 0) return best;
  for (int32_t d = -(lb - 1); d <= la - 1; ++d) {
    const uint32_t ov = ov_of[(size_t)(d + lb - 1)], mm = mm_of[(size_t)(d + lb - 1)];
    if (!(ov >= min_overlap && mm <= k && (uint64_t)mm * 1000u <= (uint64_t)permille * ov)) continue;
    bool better = best.n == 0;
    if (!better) {
      const uint64_t x = (uint64_t)mm * best.ov, y = (uint64_t)best.mm * ov;
      better = x < y || (x == y && (ov > best.ov || (ov == best.ov && d > best.d)));
    }
    const uint32_t n = best.n + 1;
    if (better) best = OvlBest{d, ov, mm, n};
    best.n = n;
  }
  return best;
}

static uint64_t n_pairs = 0, n_offsets = 0, n_bests = 0;

static void check_pair(uint32_t profile, uint32_t la, uint32_t lb, uint32_t flavour) {
  std::vector<uint8_t> a(la), r2(lb);
  for (uint8_t& c : a) c = random_byte(profile, flavour);
  for (uint8_t& c : r2) c = random_byte(profile, flavour);
  if (flavour != 1 && la && lb && below(2)) {  // a planted overlap: a's tail is b's head, with a substitution or two
    const uint32_t ov = 1 + (uint32_t)below(std::min(la, lb));
    for (uint32_t i = 0; i < ov; ++i) r2[lb - 1 - i] = (uint8_t)ovl_complement(profile, a[la - ov + i]);
    if (below(2)) r2[lb - 1 - below(ov)] = random_byte(profile, flavour);
  }
  const std::vector<uint8_t> b = reverse_complement(profile, r2);
  const uint32_t P = ovl_planes(profile);
  std::vector<uint32_t> mm_of, ov_of;
  for (int32_t d = -((int32_t)lb - 1); d <= (int32_t)la - 1 && lb > 0; ++d) {
    uint32_t ov = 0;
    mm_of.push_back(brute_mismatches(profile, a, b, d, &ov));
    ov_of.push_back(ov);
  }
  for (uint32_t W : {ovl_words(std::max(la, lb)), kOvlMaxWords}) {
    std::vector<uint32_t> ap((P + 1) * W), bp((P + 1) * 3 * W);
    ovl_encode_a(profile, a.data(), la, W, ap.data());
    ovl_encode_b(profile, r2.data(), lb, W, bp.data());
    for (int32_t d = -((int32_t)lb - 1); d <= (int32_t)la - 1 && lb > 0; ++d) {
      const uint32_t ov = ov_of[(size_t)(d + (int32_t)lb - 1)], mm = mm_of[(size_t)(d + (int32_t)lb - 1)];
      CHECK(ovl_overlap(la, lb, d) == ov && (uint32_t)(ovl_hi(la, lb, d) - ovl_lo(d)) == ov);
      const uint32_t q = ovl_shift_word(W, d);
      CHECK(q + W <= 3 * W - 1 && ovl_shift_bits(d) < 32);
      CHECK(plane_mismatches(profile, ap.data(), bp.data(), W, d) == mm);
      ++n_offsets;
    }
    // the offsets a call looks at are those that can be accepted
    for (uint32_t mo : {1u, 2u, 10u, 31u, 64u, 65u, 130u, 512u, 513u}) {
      const OvlRange range = ovl_offsets(la, lb, mo);
      uint32_t count = 0;
      int32_t first = 0;
      for (int32_t d = -((int32_t)lb - 1); d <= (int32_t)la - 1 && lb > 0; ++d)
        if (ovl_overlap(la, lb, d) >= mo) {
          if (!count) first = d;
          ++count;
          CHECK(d >= range.d_first && d < range.d_first + (int32_t)range.count);
        }
      CHECK(count == range.count && (count == 0 || first == range.d_first));
      CHECK(ovl_rounds(range.count) <= (la + lb + 62) / 64);
    }
    // the record
    for (int rep = 0; rep < 3; ++rep) {
      const uint32_t mo = rep == 0 ? 1u : 1u + (uint32_t)below(std::max(1u, std::min(la, lb)) + 2);
      const uint32_t k = rep == 1 ? 0xFFFFFFFFu : (uint32_t)below(6), permille = rep == 2 ? (uint32_t)below(1001) : (below(2) ? 1000u : 100u);
      const OvlBest got = best_as_the_kernel(profile, ap.data(), bp.data(), W, la, lb, mo, k, permille);
      const OvlBest want = best_by_definition((int32_t)la, (int32_t)lb, mm_of, ov_of, mo, k, permille);
      CHECK(got.n == want.n && got.d == want.d && got.ov == want.ov && got.mm == want.mm);
      if (want.n == 0) CHECK(got.d == 0 && got.ov == 0 && got.mm == 0);
      ++n_bests;
    }
  }
  ++n_pairs;
}

static void check_small_things() {
  for (uint32_t r = 0; r < 32; ++r) {
    const uint32_t lo = (uint32_t)rnd(), hi = (uint32_t)rnd();
    CHECK(ovl_funnel(lo, hi, r) == (r ? (lo >> r) | (hi << (32 - r)) : lo));
  }
  CHECK(ovl_words(0) == 2 && ovl_words(64) == 2 && ovl_words(65) == 4 && ovl_words(128) == 4 && ovl_words(129) == 6 && ovl_words(192) == 6);
  CHECK(ovl_words(193) == 8 && ovl_words(256) == 8 && ovl_words(257) == 16 && ovl_words(512) == 16 && kOvlMaxWords * 32 == kOvlMaxLen);
  // acceptance at its edges: equality on every side is accepted
  CHECK(ovl_accepts(1, 20, 20, 1, 50) && !ovl_accepts(2, 20, 20, 1, 1000) && !ovl_accepts(1, 20, 21, 1, 1000) && !ovl_accepts(2, 20, 20, 2, 99));
  CHECK(ovl_accepts(2, 20, 20, 2, 100) && ovl_accepts(0, 1, 1, 0, 0) && ovl_accepts(512, 512, 1, 0xFFFFFFFFu, 1000) && !ovl_accepts(512, 512, 1, 511, 1000));
  // the order: density, then the longer overlap, then the larger offset
  CHECK(ovl_better(1, 40, 0, 1, 20, 5) && !ovl_better(1, 20, 5, 1, 40, 0));      // 1/40 < 1/20
  CHECK(ovl_better(2, 40, -3, 1, 20, 7) && !ovl_better(1, 20, 7, 2, 40, -3));    // 2/40 == 1/20: the longer
  CHECK(ovl_better(0, 12, 4, 0, 12, -4) && !ovl_better(0, 12, -4, 0, 12, 4));    // mirror images: the larger d
  CHECK(ovl_better(0, 5, 0, 1, 500, 0));
  const OvlBest x{3, 10, 0, 2}, none = ovl_none();
  OvlBest c = ovl_combine(x, none);
  CHECK(c.d == 3 && c.ov == 10 && c.mm == 0 && c.n == 2);
  c = ovl_combine(none, x);
  CHECK(c.d == 3 && c.ov == 10 && c.mm == 0 && c.n == 2);
  c = ovl_combine(none, none);
  CHECK(c.d == 0 && c.ov == 0 && c.mm == 0 && c.n == 0);
}

// every refusal as the pair (the call's own code, the gate's code)
static uint64_t check_refusals() {
  OvlCall ok{};
  ok.have_searcher = ok.have_out = true;
  ok.min_overlap = 10; ok.max_permille = 200;
  ok.n1 = ok.n2 = 7;
  ReadsGate& g = ok.gate;
  g.handles = 2;
  g.have_reads[0] = g.have_reads[1] = g.handle_read = true;
  g.profile = kHamDna;
  g.longest[0] = 512; g.longest[1] = 150;
  g.device_s = g.device_r[0] = g.device_r[1] = 1;
  ReadsRefusal gate = kRdsTooLong;
  CHECK(ovl_refusal(ok, &gate) == kOvlOk && gate == kRdsOk);
  uint64_t n = 0;
  auto refused = [&](OvlRefusal want, ReadsRefusal want_gate, auto&& change) {
    OvlCall c = ok;
    change(c);
    ReadsRefusal got = kRdsTooLong;
    CHECK(ovl_refusal(c, &got) == want && got == want_gate);
    ++n;
  };
  refused(kOvlNullSearcher, kRdsOk, [](OvlCall& c) { c.have_searcher = false; c.flags = 1; });
  refused(kOvlFlags, kRdsOk, [](OvlCall& c) { c.flags = 1u << 20; c.min_overlap = 0; });
  refused(kOvlMinOverlap, kRdsOk, [](OvlCall& c) { c.min_overlap = 0; c.max_permille = 1001; });
  refused(kOvlPermille, kRdsOk, [](OvlCall& c) { c.max_permille = 1001; c.gate.profile = 0; });
  refused(kOvlGate, kRdsAscii, [](OvlCall& c) { c.gate.profile = 0; c.gate.overhang = true; });
  refused(kOvlGate, kRdsAscii, [](OvlCall& c) { c.gate.profile = kHamAsciiCi; });
  refused(kOvlGate, kRdsOverhang, [](OvlCall& c) { c.gate.profile = kHamIupac; c.gate.overhang = c.gate.only_best = true; });
  refused(kOvlGate, kRdsOnlyBest, [](OvlCall& c) { c.gate.only_best = c.gate.max_n_frac = true; });
  refused(kOvlGate, kRdsNFrac, [](OvlCall& c) { c.gate.max_n_frac = true; c.gate.have_reads[0] = false; });
  refused(kOvlGate, kRdsNullReads, [](OvlCall& c) { c.gate.have_reads[0] = false; c.n1 = 0; });
  refused(kOvlGate, kRdsNullReads, [](OvlCall& c) { c.gate.have_reads[1] = false; });
  refused(kOvlCounts, kRdsOk, [](OvlCall& c) { c.n2 = 8; c.gate.device_r[0] = 0; });
  refused(kOvlGate, kRdsDevice, [](OvlCall& c) { c.gate.device_r[0] = 0; c.gate.longest[0] = 513; });
  refused(kOvlGate, kRdsDevice, [](OvlCall& c) { c.gate.device_r[1] = 2; });
  refused(kOvlGate, kRdsDevice, [](OvlCall& c) { c.gate.device_s = 0; });
  refused(kOvlGate, kRdsTooLong, [](OvlCall& c) { c.gate.longest[0] = 513; c.have_out = false; });
  refused(kOvlGate, kRdsTooLong, [](OvlCall& c) { c.gate.longest[1] = 1ull << 40; });
  refused(kOvlNullOut, kRdsOk, [](OvlCall& c) { c.have_out = false; });
  refused(kOvlOk, kRdsOk, [](OvlCall& c) { c.have_out = false; c.n1 = c.n2 = 0; });          // zero pairs need no `out`
  refused(kOvlOk, kRdsOk, [](OvlCall& c) { c.gate.profile = kHamIupac; c.max_permille = 1000; c.min_overlap = 0xFFFFFFFFu; });
  // the tickets are not this function's: the entry points look at them behind all of it
  refused(kOvlOk, kRdsOk, [](OvlCall& c) { c.gate.in_flight = true; });
  // before the handles are read nothing of theirs is judged
  refused(kOvlOk, kRdsOk, [](OvlCall& c) { c.gate.handle_read = false; c.gate.device_r[0] = 0; c.gate.longest[1] = 513; });
  return n;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "complement")) {
    for (uint32_t profile : {kHamDna, kHamIupac}) {
      printf("%s ", profile == kHamDna ? "dna" : "iupac");
      for (uint32_t c = 0; c < 256; ++c) printf("%02x", ovl_complement(profile, c));
      printf("\n");
    }
    return 0;
  }
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  check_small_things();
  const uint64_t refusals = check_refusals();
  std::vector<uint32_t> all;
  for (uint32_t l = 0; l <= 130; ++l) all.push_back(l);
  for (uint32_t l : {191u, 192u, 193u, 511u, 512u}) all.push_back(l);
  const uint32_t borders[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 100, 130, 191, 192, 193, 511, 512};
  for (uint32_t profile : {kHamDna, kHamIupac})
    for (uint32_t l : all) {
      const bool wide = l > 193;
      for (uint32_t other : borders) {
        if (wide && other > 193 && other != l) continue;  // (512 x 511 once is enough: the pair below)
        check_pair(profile, l, other, (uint32_t)below(3));
        if (other != l) check_pair(profile, other, l, (uint32_t)below(3));
      }
      check_pair(profile, l, l, 2);
      check_pair(profile, l, all[below(all.size())], 1);
    }
  for (uint32_t profile : {kHamDna, kHamIupac}) {
    check_pair(profile, 512, 511, 0);
    check_pair(profile, 511, 512, 2);
  }
  printf("ok pairs=%llu offsets=%llu bests=%llu refusals=%llu\n", (unsigned long long)n_pairs, (unsigned long long)n_offsets, (unsigned long long)n_bests,
         (unsigned long long)refusals);
  return 0;
}
