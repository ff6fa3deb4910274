// merge_step_driver.cc -- drives sassy_amd/csrc/merge_step.h (the arithmetic of sassy_hip_merge_pairs, free of HIP) on the
// host against a byte-wise brute force of the definition: for every (la, lb) in 0 .. 70, and for the lengths 127, 128, 129,
// 511 and 512 against the border lengths, at EVERY offset that has an overlap, Dna and Iupac, the merged length and every
// 64-byte block of the merged text and quality as merge_write_kernel builds them -- a's bytes as aligned 16-byte pieces,
// R2's bytes as five 16-byte pieces from an address of any alignment and sign, shifted by fq_shift_block and word-reversed,
// then mrg_word -- out of buffers whose pads and neighbours hold garbage, with every piece bounded as the kernel bounds it;
// mrg_sources at every column; all 256 x 256 quality pairs through mrg_consensus with equal and with unequal bytes; every
// refusal, in its order.  Built by tests/test_merge_pairs_cpu.py with -fsanitize=address,undefined.
//   merge_step_driver <seed>    prints "ok pairs=<n> offsets=<n> columns=<n> consensus=<n> refusals=<n>", exit status 0;
//                               a failed check: its line on stderr, 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sassy_amd/csrc/fastq_step.h"  // (fq_shift_block, which the write kernel shifts R2's bytes with)
#include "../../sassy_amd/csrc/merge_step.h"

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

static uint8_t random_base(uint32_t profile) {
  static const char iupac[] = "ACGTUNRYSWKMBDHVXacgtunry-";
  static const char dna[] = "ACGTacgt";
  if (profile == kHamIupac) return below(16) ? (uint8_t)iupac[below(sizeof(iupac) - 1)] : (uint8_t)below(256);
  return below(16) ? (uint8_t)dna[below(sizeof(dna) - 1)] : (uint8_t)below(256);
}

// ---- the definition, byte by byte, with branches ----
static void brute_consensus(uint8_t ca, uint8_t qa, uint8_t cb, uint8_t qb, uint8_t* c, uint8_t* q) {
  if (ca == cb) {
    *c = ca;
    *q = std::max(qa, qb);
    return;
  }
  *c = qb > qa ? cb : ca;
  const int diff = qa > qb ? qa - qb : qb - qa;
  *q = (uint8_t)std::min(126, 33 + std::max(2, diff));
}
struct Merged {
  std::vector<uint8_t> text, qual;
};
// rec: (d, ov, mm, n)
static Merged brute_merge(uint32_t profile, const std::vector<uint8_t>& r1, const std::vector<uint8_t>& q1, const std::vector<uint8_t>& r2,
                          const std::vector<uint8_t>& q2, int32_t d, uint32_t ov, uint32_t n) {
  Merged m;
  if (n == 0) return m;
  const int32_t la = (int32_t)r1.size(), lb = (int32_t)r2.size();
  std::vector<uint8_t> b(r2.size()), qb(r2.size());
  for (int32_t t = 0; t < lb; ++t) {
    b[(size_t)t] = (uint8_t)ovl_complement(profile, r2[(size_t)(lb - 1 - t)]);
    qb[(size_t)t] = q2[(size_t)(lb - 1 - t)];
  }
  const int32_t L = d >= 0 ? std::max(la, d + lb) : (int32_t)ov;
  for (int32_t p = 0; p < L; ++p) {
    const int32_t j = p - d;
    const bool in_a = p < la, in_b = j >= 0 && j < lb;
    CHECK(in_a || in_b);
    uint8_t c, q;
    if (in_a && in_b) brute_consensus(r1[(size_t)p], q1[(size_t)p], b[(size_t)j], qb[(size_t)j], &c, &q);
    else if (in_a) c = r1[(size_t)p], q = q1[(size_t)p];
    else c = b[(size_t)j], q = qb[(size_t)j];
    m.text.push_back(c);
    m.qual.push_back(q);
  }
  return m;
}

// ---- a read inside a buffer as a handle holds it: from a multiple of 64 on, garbage around it ----
struct Buffer {
  std::vector<uint8_t> text, qual;  // sizes a multiple of 64
  uint64_t start = 0;
};
static Buffer place(const std::vector<uint8_t>& seq, const std::vector<uint8_t>& q, uint64_t blocks_in_front) {
  Buffer B;
  B.start = 64 * blocks_in_front;
  const uint64_t size = B.start + (seq.size() + 63) / 64 * 64 + 64;
  B.text.resize(size);
  B.qual.resize(size);
  for (uint64_t i = 0; i < size; ++i) B.text[i] = (uint8_t)below(256), B.qual[i] = (uint8_t)below(256);
  std::copy(seq.begin(), seq.end(), B.text.begin() + (ptrdiff_t)B.start);
  std::copy(q.begin(), q.end(), B.qual.begin() + (ptrdiff_t)B.start);
  return B;
}

// ---- the write kernel's way to one block (merge_pairs.hip: load_shifted64, load_aligned16, the loop over mrg_word) ----
static void load_aligned16(const std::vector<uint8_t>& base, uint64_t at, uint32_t (&w)[4]) {
  CHECK(at % 16 == 0);
  for (int i = 0; i < 4; ++i) w[i] = 0;
  if (at < base.size()) {
    CHECK(at + 16 <= base.size());
    memcpy(w, base.data() + at, 16);
  }
}
static void load_shifted64(const std::vector<uint8_t>& base, int64_t src, uint32_t (&out)[16]) {
  const int64_t al = src & ~(int64_t)15;
  uint32_t w[20];
  for (int j = 0; j < 5; ++j) {
    const int64_t at = al + 16 * j;
    uint32_t v[4] = {0, 0, 0, 0};
    if (at >= 0 && (uint64_t)at < base.size()) {
      CHECK((uint64_t)at + 16 <= base.size());
      memcpy(v, base.data() + at, 16);
    }
    for (int i = 0; i < 4; ++i) w[4 * j + i] = v[i];
  }
  fq_shift_block(w, (uint32_t)(src & 15), 64u, out);
}
static void block_as_the_kernel(uint32_t profile, const Buffer& A, uint32_t la, const Buffer& B, uint32_t lb, int32_t d, uint32_t len, uint32_t pb,
                                uint8_t* out_t, uint8_t* out_q) {
  uint32_t wb[16], qb[16];
  const int64_t b_at = (int64_t)B.start + mrg_r2_first(pb, lb, d);
  load_shifted64(B.text, b_at, wb);
  load_shifted64(B.qual, b_at, qb);
  for (int q = 0; q < 4; ++q) {
    uint32_t wa[4], qa[4];
    load_aligned16(A.text, A.start + pb + 16u * q, wa);
    load_aligned16(A.qual, A.start + pb + 16u * q, qa);
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * q + i;
      const MrgWord w = mrg_word(profile, pb + 4u * j, la, lb, d, len, wa[i], qa[i], mrg_reverse_word(wb[15 - j]), mrg_reverse_word(qb[15 - j]));
      memcpy(out_t + 4 * j, &w.text, 4);
      memcpy(out_q + 4 * j, &w.qual, 4);
    }
  }
}

static uint64_t n_pairs, n_offsets, n_columns;

static void check_pair(uint32_t profile, uint32_t la, uint32_t lb) {
  std::vector<uint8_t> r1(la), q1(la), r2(lb), q2(lb);
  for (auto& c : r1) c = random_base(profile);
  for (auto& c : r2) c = random_base(profile);
  for (auto& c : q1) c = (uint8_t)(below(8) ? 33 + below(42) : below(256));
  for (auto& c : q2) c = (uint8_t)(below(8) ? 33 + below(42) : below(256));
  // (the alphabets are small: inside every overlap some columns agree and some do not)
  const Buffer A = place(r1, q1, below(2)), B = place(r2, q2, below(2));
  ++n_pairs;
  // not merged: whatever the other fields say
  CHECK(mrg_length(la, lb, OvlBest{3, 5, 1, 0u}) == 0u && mrg_length(la, lb, ovl_none()) == 0u);
  if (la == 0 || lb == 0) return;
  for (int32_t d = -(int32_t)(lb - 1); d <= (int32_t)la - 1; ++d) {  // every offset that has an overlap
    const uint32_t ov = ovl_overlap(la, lb, d);
    CHECK(ov >= 1);
    const OvlBest rec{d, ov, 0u, 1u + (uint32_t)below(3)};
    const Merged want = brute_merge(profile, r1, q1, r2, q2, d, ov, rec.n);
    const uint32_t L = mrg_length(la, lb, rec);
    CHECK(L == want.text.size() && L >= ov && L <= la + lb);
    ++n_offsets;
    for (uint32_t p = 0; p < L; ++p) {
      const MrgSources s = mrg_sources(p, la, lb, d);
      const int32_t j = (int32_t)p - d;
      CHECK(s.in_a == (p < la) && s.in_b == (j >= 0 && j < (int32_t)lb) && (s.in_a || s.in_b));
      CHECK((!s.in_a || s.i == p) && (!s.in_b || s.j == (uint32_t)j));
      if (d < 0) CHECK(s.in_a && s.in_b);  // read-through: both cover every column
    }
    for (uint32_t pb = 0; pb < L; pb += 64) {
      uint8_t t[64], q[64];
      block_as_the_kernel(profile, A, la, B, lb, d, L, pb, t, q);
      for (uint32_t i = 0; i < 64; ++i) {
        const uint32_t p = pb + i;
        const uint8_t wt = p < L ? want.text[p] : 0, wq = p < L ? want.qual[p] : 0;
        if (t[i] != wt || q[i] != wq) {
          fprintf(stderr, "profile %u la %u lb %u d %d column %u: got %u/%u, want %u/%u\n", profile, la, lb, d, p, t[i], q[i], wt, wq);
          exit(1);
        }
        ++n_columns;
      }
    }
  }
}

static uint64_t check_consensus() {
  uint64_t n = 0;
  static const uint8_t bytes[][2] = {{'A', 'A'}, {'A', 'C'}, {'N', 'A'}, {'a', 'A'}, {0, 255}, {255, 255}, {'T', 'G'}};
  for (const auto& cc : bytes)
    for (uint32_t qa = 0; qa < 256; ++qa)
      for (uint32_t qb = 0; qb < 256; ++qb) {
        uint8_t c, q;
        brute_consensus(cc[0], (uint8_t)qa, cc[1], (uint8_t)qb, &c, &q);
        const MrgByte got = mrg_consensus(cc[0], qa, cc[1], qb);
        CHECK(got.c == c && got.q == q);
        const MrgByte both = mrg_column(true, true, cc[0], qa, cc[1], qb), only_a = mrg_column(true, false, cc[0], qa, cc[1], qb),
                      only_b = mrg_column(false, true, cc[0], qa, cc[1], qb), none = mrg_column(false, false, cc[0], qa, cc[1], qb);
        CHECK(both.c == c && both.q == q && only_a.c == cc[0] && only_a.q == qa && only_b.c == cc[1] && only_b.q == qb && none.c == 0 && none.q == 0);
        ++n;
      }
  // the corners by hand: a tie keeps a's byte; differences of 0, 1, 2 give 35, of 93 gives 126, of more stays 126
  CHECK(mrg_consensus('A', 40, 'C', 40).c == 'A' && mrg_consensus('A', 40, 'C', 40).q == 35);
  CHECK(mrg_consensus('A', 40, 'C', 41).c == 'C' && mrg_consensus('A', 40, 'C', 41).q == 35);
  CHECK(mrg_consensus('A', 42, 'C', 40).c == 'A' && mrg_consensus('A', 42, 'C', 40).q == 35);
  CHECK(mrg_consensus('A', 43, 'C', 40).q == 36 && mrg_consensus('A', 126, 'C', 33).q == 126 && mrg_consensus('A', 33, 'C', 127).q == 126);
  CHECK(mrg_consensus('A', 33, 'A', 74).q == 74 && mrg_consensus('A', 74, 'A', 33).q == 74 && mrg_consensus('A', 50, 'A', 50).q == 50);
  return n;
}

// every refusal as (the merge's code, the overlap's code, the gate's code)
static uint32_t check_refusals() {
  uint32_t n = 0;
  MrgCall ok{};
  ok.ovl.have_searcher = ok.ovl.have_out = true;
  ok.ovl.min_overlap = 10; ok.ovl.max_permille = 200;
  ok.ovl.n1 = ok.ovl.n2 = 5;
  ReadsGate& g = ok.ovl.gate;
  g.handles = 2;
  g.have_reads[0] = g.have_reads[1] = g.handle_read = true;
  g.profile = kHamDna;
  g.longest[0] = g.longest[1] = 512;
  ok.qual1 = ok.qual2 = true; ok.have_merged = true;
  OvlRefusal why = kOvlFlags;
  ReadsRefusal gate = kRdsTooLong;
  CHECK(mrg_refusal(ok, &why, &gate) == kMrgOk && why == kOvlOk && gate == kRdsOk);
  auto expect = [&](MrgCall c, MrgRefusal want, OvlRefusal want_ovl, ReadsRefusal want_gate = kRdsOk) {
    OvlRefusal w = kOvlFlags;
    ReadsRefusal gw = kRdsTooLong;
    CHECK(mrg_refusal(c, &w, &gw) == want && w == want_ovl && gw == want_gate);
    // whatever read_overlaps refuses comes first: the merge's own two never hide it
    c.qual1 = false; c.have_merged = false;
    if (want == kMrgOverlap) CHECK(mrg_refusal(c, &w, &gw) == kMrgOverlap && w == want_ovl && gw == want_gate);
    ++n;
  };
  MrgCall c = ok;
  c.ovl.have_searcher = false; expect(c, kMrgOverlap, kOvlNullSearcher);
  c = ok; c.ovl.flags = 32; expect(c, kMrgOverlap, kOvlFlags);
  c = ok; c.ovl.min_overlap = 0; expect(c, kMrgOverlap, kOvlMinOverlap);
  c = ok; c.ovl.max_permille = 1001; expect(c, kMrgOverlap, kOvlPermille);
  c = ok; c.ovl.gate.profile = 0; expect(c, kMrgOverlap, kOvlGate, kRdsAscii);
  c = ok; c.ovl.gate.profile = kHamAsciiCi; expect(c, kMrgOverlap, kOvlGate, kRdsAscii);
  c = ok; c.ovl.gate.overhang = true; expect(c, kMrgOverlap, kOvlGate, kRdsOverhang);
  c = ok; c.ovl.gate.only_best = true; expect(c, kMrgOverlap, kOvlGate, kRdsOnlyBest);
  c = ok; c.ovl.gate.max_n_frac = true; expect(c, kMrgOverlap, kOvlGate, kRdsNFrac);
  c = ok; c.ovl.gate.have_reads[0] = false; expect(c, kMrgOverlap, kOvlGate, kRdsNullReads);
  c = ok; c.ovl.gate.have_reads[1] = false; expect(c, kMrgOverlap, kOvlGate, kRdsNullReads);
  c = ok; c.ovl.n2 = 4; expect(c, kMrgOverlap, kOvlCounts);
  c = ok; c.ovl.gate.device_r[1] = 1; expect(c, kMrgOverlap, kOvlGate, kRdsDevice);
  c = ok; c.ovl.gate.longest[0] = 513; expect(c, kMrgOverlap, kOvlGate, kRdsTooLong);
  c = ok; c.ovl.gate.longest[1] = 513; expect(c, kMrgOverlap, kOvlGate, kRdsTooLong);
  // the merge's own, in their order: the qualities, then the place for the handle
  c = ok; c.qual1 = false; expect(c, kMrgNoQuality, kOvlOk);
  c = ok; c.qual2 = false; expect(c, kMrgNoQuality, kOvlOk);
  c = ok; c.qual2 = false; c.have_merged = false; expect(c, kMrgNoQuality, kOvlOk);
  c = ok; c.have_merged = false; expect(c, kMrgNullMerged, kOvlOk);
  // before the handles are read their qualities are not asked for
  c = ok; c.ovl.gate.handle_read = false; c.qual1 = c.qual2 = false; expect(c, kMrgOk, kOvlOk);
  c.have_merged = false; expect(c, kMrgNullMerged, kOvlOk);
  return n;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  static const uint32_t borders[] = {0, 1, 63, 64, 65, 127, 128, 129, 511, 512};
  static const uint32_t longs[] = {127, 128, 129, 511, 512};
  for (uint32_t profile : {kHamDna, kHamIupac}) {
    for (uint32_t la = 0; la <= 70; ++la)
      for (uint32_t lb = 0; lb <= 70; ++lb) check_pair(profile, la, lb);
    for (uint32_t l : longs)
      for (uint32_t o : borders) {
        check_pair(profile, l, o);
        check_pair(profile, o, l);
      }
  }
  CHECK(mrg_reverse_word(0x04030201u) == 0x01020304u);
  CHECK(mrg_r2_first(0, 64, 0) == 0 && mrg_r2_first(64, 64, 0) == -64 && mrg_r2_first(0, 5, -3) == -62);
  const uint64_t consensus = check_consensus();
  const uint32_t refusals = check_refusals();
  printf("ok pairs=%llu offsets=%llu columns=%llu consensus=%llu refusals=%u\n", (unsigned long long)n_pairs, (unsigned long long)n_offsets,
         (unsigned long long)n_columns, (unsigned long long)consensus, refusals);
  return 0;
}
