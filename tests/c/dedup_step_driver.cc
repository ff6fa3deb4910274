// dedup_step_driver.cc -- dedup_step.h as the kernels of dedup_reads.hip call it, on the host, against pairs_encode of the
// byte-wise extracted window.  A stand-alone program with its own main and no HIP: tests/test_dedup_reads_cpu.py builds it with
// the host compiler under AddressSanitizer and UBSan and runs it.  A lane of dedup_encode_kernel is simulated word for word --
// the window through ddp_window_planes out of a text whose pads hold garbage, the first pairs_words(m) words of every plane
// stored at [p W + w], both strands of the target record -- for every key length, window place, read length, end and profile
// the kernels can meet; then the quality sum as dedup_score_kernel's lanes share it, the score key as a max-reduction in any
// order, and every refusal in its order.  Prints "ok" and what it counted; any difference ends it with 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sassy_amd/csrc/dedup_step.h"

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

struct Counts {
  long cases = 0, windows = 0, no_window = 0, strands = 0, refusals = 0, reductions = 0, sums = 0;
};

// one lane of dedup_encode_kernel<P, IUPAC, true>: what it stores for the entry and for both strands of the target record
template <int P, bool IUPAC>
static bool lane(const Text& t, uint64_t read, uint32_t m, uint32_t at, bool end3, std::vector<uint32_t>& a, std::vector<uint32_t>& t0,
                 std::vector<uint32_t>& t1) {
  constexpr uint32_t profile = IUPAC ? kHamIupac : kHamDna;
  const uint64_t s0 = t.start[read], l = t.len[read], bytes = t.bytes.size();
  const bool fits = l <= kOvlMaxLen && s0 <= bytes && l <= bytes - s0;
  const uint32_t la = fits ? (uint32_t)l : 0u;
  if (!dmx_has_window(la, at, m)) return false;
  const uint32_t W = pairs_words(m);
  uint32_t fw[P][4], rv[P][4], fw1[P][4], rv1[P][4];
  const Loader load{t.bytes.data(), bytes};
  ddp_window_planes<P, true>(profile, load, s0 + dmx_window(la, at, m, end3), bytes, m, fw, rv);
  ddp_window_planes<P, false>(profile, load, s0 + dmx_window(la, at, m, end3), bytes, m, fw1, rv1);  // (one strand: the same entry)
  a.assign(P * W, 0xDEADBEEFu); t0.assign(P * W, 0xDEADBEEFu); t1.assign(P * W, 0xDEADBEEFu);
  for (int p = 0; p < P; ++p)
    for (int w = 0; w < 4; ++w) {
      CHECK(fw[p][w] == fw1[p][w] && rv1[p][w] == 0u, p, w);
      if ((uint32_t)w < W) {
        a[p * W + w] = fw[p][w];
        t0[p * W + w] = fw[p][w];
        t1[p * W + w] = rv[p][w];
      } else {
        CHECK(fw[p][w] == 0u && rv[p][w] == 0u, p, w);  // (what is not stored holds nothing)
      }
    }
  return true;
}

static void walk_cases(uint32_t profile, Counts& n) {
  const uint32_t ms[] = {1, 8, 31, 32, 33, 63, 64, 65, 96, 127, 128};
  std::vector<uint32_t> ats;
  for (uint32_t a = 0; a < 16; ++a) ats.push_back(a);  // every residue mod 16
  for (uint32_t a : {63u, 64u, 65u, 127u, 128u, 129u, 383u, 384u, 385u}) ats.push_back(a);  // at and across 64, 128 and 384
  const uint32_t P = pairs_planes(profile);
  for (uint32_t m : ms)
    for (uint32_t at : ats) {
      if (at + m > kOvlMaxLen) continue;
      for (int end3 = 0; end3 < 2; ++end3) {
        std::vector<std::vector<uint8_t>> reads;
        for (uint32_t la : {at + m - 1, at + m, at + m + 1, 0u, 512u}) {
          if (la > kOvlMaxLen) continue;  // (no batch holds such a read: the call refuses it)
          std::vector<uint8_t> r(la);
          for (auto& c : r) c = letter(profile);
          reads.push_back(r);
        }
        const Text t = lay_out(reads);
        for (uint64_t r = 0; r < reads.size(); ++r) {
          ++n.cases;
          std::vector<uint32_t> a, t0, t1;
          const bool has = profile == kHamIupac ? lane<4, true>(t, r, m, at, end3 != 0, a, t0, t1) : lane<2, false>(t, r, m, at, end3 != 0, a, t0, t1);
          const uint32_t la = (uint32_t)reads[r].size();
          CHECK(has == (at + m <= la), (long)la, at, m);
          if (!has) {
            ++n.no_window;
            continue;
          }
          ++n.windows;
          // the window byte by byte, then the host's own encoding of it and of its reverse complement
          const uint32_t w0 = end3 ? la - at - m : at, W = pairs_words(m);
          std::vector<uint8_t> win(reads[r].begin() + w0, reads[r].begin() + w0 + m), rev(m);
          pairs_reverse_complement(win.data(), m, [&](uint8_t c) { return (uint8_t)ovl_complement(profile, c); }, rev.data());
          std::vector<uint32_t> want(P * W), want_rev(P * W);
          pairs_encode(profile, win.data(), m, W, want.data());
          pairs_encode(profile, rev.data(), m, W, want_rev.data());
          CHECK(a == want && t0 == want, m, at, (long)la);
          CHECK(t1 == want_rev, m, at, (long)la);
          n.strands += 2;
        }
      }
    }
}

// the quality sum as kDdpScoreLanes lanes share a read, out of a buffer whose pads hold garbage
static void walk_sums(Counts& n) {
  for (uint32_t la : {0u, 1u, 15u, 16u, 17u, 63u, 64u, 65u, 127u, 128u, 129u, 150u, 255u, 256u, 500u, 511u, 512u}) {
    std::vector<std::vector<uint8_t>> reads(3);
    for (auto& c : reads[0] = std::vector<uint8_t>(rnd_below(200))) c = (uint8_t)rnd_below(256);
    for (auto& c : reads[1] = std::vector<uint8_t>(la)) c = (uint8_t)(la % 2 ? 255u : rnd_below(256));
    for (auto& c : reads[2] = std::vector<uint8_t>(rnd_below(200))) c = (uint8_t)rnd_below(256);
    const Text t = lay_out(reads);
    const Loader load{t.bytes.data(), t.bytes.size()};
    uint32_t want = 0, got = 0, loads = 0;
    for (uint8_t c : reads[1]) want += c;
    for (uint32_t q = 0; q < kDdpScoreLanes; ++q)
      for (uint32_t piece = q; piece < ddp_pieces(la); piece += kDdpScoreLanes) {
        uint32_t w[4];
        load(t.start[1] + 16u * piece, w);
        got += ddp_piece_sum(w, piece, la);
        ++loads;
      }
    CHECK(got == want && loads == (la + 15) / 16, (long)la, got, want);
    ++n.sums;
  }
  CHECK(ddp_byte_sum(0xFFFFFFFFu) == 1020u && ddp_byte_sum(0x01020304u) == 10u && ddp_byte_sum(0u) == 0u);
}

// the key: a max-reduction in any order names the highest score's smallest index
static void walk_reductions(Counts& n) {
  for (int round = 0; round < 2000; ++round) {
    const uint32_t count = 1 + rnd_below(40);
    std::vector<uint32_t> score(count), index(count), order(count);
    for (uint32_t i = 0; i < count; ++i) {
      score[i] = round % 3 == 0 ? rnd_below(3) : round % 3 == 1 ? 130560u - rnd_below(2) : rnd();
      index[i] = round % 2 ? i * 7u + rnd_below(7) : 0xFFFFFFFEu - (i * 5u + rnd_below(5));  // distinct; the largest a call can hold among them
      order[i] = i;
    }
    uint32_t want = 0;
    for (uint32_t i = 1; i < count; ++i)
      if (score[i] > score[want] || (score[i] == score[want] && index[i] < index[want])) want = i;
    for (int shuffle = 0; shuffle < 3; ++shuffle) {
      for (uint32_t i = count; i > 1; --i) std::swap(order[i - 1], order[rnd_below(i)]);
      uint64_t best = 0;  // (what a group's cell holds before its first read)
      for (uint32_t i : order) best = std::max(best, ddp_key(score[i], index[i]));
      CHECK(best != 0 && ddp_key_read(best) == index[want] && (uint32_t)(best >> 32) == score[want], round, (long)index[want]);
    }
    ++n.reductions;
  }
}

// every refusal as the pair (the call's own code, the gate's code)
static void walk_refusals(Counts& n) {
  DdpCall ok{};
  ok.have_searcher = true; ok.flags = kDdpEnd3; ok.method = 2; ok.at = 384; ok.m = 128; ok.have_out = true;
  ok.gate.handles = 1; ok.gate.profile = kHamDna;
  ok.gate.have_reads[0] = true; ok.gate.handle_read = true; ok.gate.device_s = 1; ok.gate.device_r[0] = 1; ok.gate.longest[0] = 512;
  ReadsRefusal gate = kRdsTooLong;
  CHECK(ddp_refusal(ok, &gate) == kDdpOk && gate == kRdsOk);
  ++n.refusals;
  // everything wrong at once: taking the faults away one at a time from the front shows each refusal in its place
  DdpCall c = ok;
  ReadsGate& g = c.gate;
  c.have_searcher = false; c.flags = 2; c.method = 3; c.m = 0; c.at = 600; g.profile = 0; g.overhang = g.only_best = g.max_n_frac = true;
  g.have_reads[0] = false; g.device_r[0] = 0; g.longest[0] = 513; c.have_out = false; g.in_flight = true;
  const auto expect = [&](DdpRefusal want, ReadsRefusal want_gate = kRdsOk) {
    ReadsRefusal got_gate = kRdsTooLong;
    const DdpRefusal got = ddp_refusal(c, &got_gate);
    CHECK(got == want && got_gate == want_gate, (long)got, (long)want, (long)got_gate);
    ++n.refusals;
  };
  expect(kDdpNullSearcher); c.have_searcher = true;
  expect(kDdpFlags); c.flags = 3; expect(kDdpFlags); c.flags = 1;
  expect(kDdpMethod); c.method = 0;
  expect(kDdpLen); c.m = 129; expect(kDdpLen); c.m = 1;
  expect(kDdpAt); c.at = 512; expect(kDdpAt); c.at = 511;
  expect(kDdpGate, kRdsAscii); g.profile = kHamAsciiCi; expect(kDdpGate, kRdsAscii); g.profile = kHamIupac;
  expect(kDdpGate, kRdsOverhang); g.overhang = false;
  expect(kDdpGate, kRdsOnlyBest); g.only_best = false;
  expect(kDdpGate, kRdsNFrac); g.max_n_frac = false;
  expect(kDdpGate, kRdsNullReads); g.have_reads[0] = true;
  g.handle_read = false;
  expect(kDdpNullOut);  // (the handle's fields count only once they were read)
  g.handle_read = true;
  expect(kDdpGate, kRdsDevice); g.device_r[0] = 1;
  expect(kDdpGate, kRdsTooLong); g.longest[0] = 512;
  expect(kDdpNullOut); c.have_out = true;
  expect(kDdpGate, kRdsInFlight); g.in_flight = false;
  expect(kDdpOk);
}

int main() {
  Counts n;
  walk_cases(kHamDna, n);
  walk_cases(kHamIupac, n);
  walk_sums(n);
  walk_reductions(n);
  walk_refusals(n);
  // the reversal alone, at every length
  for (uint32_t m = 1; m <= 128; ++m) {
    uint32_t in[4], out[4];
    for (auto& w : in) w = rnd() ^ (rnd() << 16);
    for (uint32_t w = 0; w < 4; ++w) in[w] &= pairs_row_mask(m, w);
    ddp_reverse_rows(in, m, out);
    for (uint32_t t = 0; t < 128; ++t) {
      const uint32_t got = (out[t >> 5] >> (t & 31)) & 1u;
      const uint32_t want = t < m ? (in[(m - 1 - t) >> 5] >> ((m - 1 - t) & 31)) & 1u : 0u;
      CHECK(got == want, m, t);
    }
  }
  std::printf("ok cases=%ld windows=%ld no_window=%ld strands=%ld sums=%ld reductions=%ld refusals=%ld\n", n.cases, n.windows, n.no_window, n.strands,
              n.sums, n.reductions, n.refusals);
  return 0;
}
