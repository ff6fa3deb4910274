// trim_step_driver.cc -- drives sassy_amd/csrc/trim_step.h (the arithmetic of sassy_hip_trim_reads and sassy_hip_reads_slice,
// free of HIP) on the host, as trim_find_kernel and reads_window_write_kernel call it -- 64 lanes simulated in loops, ballots
// and shuffles as arrays -- against a byte-wise brute force of the definition:
//   for every read length 0 .. 130, 191 .. 193, 255 .. 257, 511, 512, adapter lengths 1, 31, 32, 33, 63, 64, both profiles, the
//   word count the kernel would take and the widest (16): the adapter planted at EVERY position of the read (so it runs off
//   the end at every prefix length) among up to two other adapters, under random min_overlap, k, max_permille, quality_cutoff,
//   min_length and substitutions, and once not planted at all; the whole record compared;
//   the quality walk alone on all-low, all-high, all-tie and random qualities at every length;
//   every refusal of trm_refusal in its order;
//   every 64-byte block of a window [begin, begin + len) of a read out of a garbage-padded buffer, begin at every residue
//   mod 16, with every 16-byte piece asserted inside its buffer.
// Built by tests/test_trim_reads_cpu.py with -fsanitize=address,undefined.
//   trim_step_driver <seed>    prints "ok reads=<n> positions=<n> walks=<n> refusals=<n> blocks=<n>", exit status 0;
//                              a failed check: its line on stderr, 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sassy_amd/csrc/trim_step.h"

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
  return (uint8_t)dna[below(sizeof(dna) - 1)];
}

struct Params {
  uint32_t min_overlap, k, max_permille, cutoff, min_length;
};
typedef std::vector<uint8_t> Bytes;

// ---- the definition, byte by byte, with branches ----
static uint32_t brute_quality(const Bytes& q, uint32_t cutoff) {
  const uint32_t la = (uint32_t)q.size();
  if (cutoff == 0) return la;
  int s = 0, mn = 0;
  uint32_t lq = la;
  for (uint32_t i = la; i-- > 0;) {
    s += (int)q[i] - 33 - (int)cutoff;
    if (s > 0) break;
    if (s < mn) {
      mn = s;
      lq = i;
    }
  }
  return lq;
}
static TrmRecord brute_trim(uint32_t profile, const Bytes& a, const Bytes& q, const std::vector<Bytes>& ads, const Params& p) {
  const uint32_t lq = brute_quality(q, p.cutoff);
  bool found = false;
  uint32_t bc = 0, bov = 0, bmm = 0, bj = 0;
  for (uint32_t c = 0; c < lq && !found; ++c) {  // the smallest c first: what is accepted there decides among itself
    for (uint32_t j = 0; j < ads.size(); ++j) {
      const uint32_t m = (uint32_t)ads[j].size(), ov = std::min(m, lq - c);
      uint32_t mm = 0;
      for (uint32_t i = 0; i < ov; ++i) mm += ham_match(profile, ads[j][i], a[c + i]) ? 0u : 1u;
      if (ov < p.min_overlap || mm > p.k || mm * 1000u > p.max_permille * ov) continue;
      bool better = !found;
      if (found) {
        if (mm * bov != bmm * ov) better = mm * bov < bmm * ov;
        else if (ov != bov) better = ov > bov;
        else better = false;  // (j ascends)
      }
      if (better) found = true, bc = c, bov = ov, bmm = mm, bj = j;
    }
  }
  const uint32_t cut = found ? bc : lq;
  TrmRecord r;
  r.length = cut >= p.min_length ? cut : 0u;
  r.quality_len = lq;
  r.adapter_pos = cut;
  r.tail = (found ? bj : 0xFFFFu) | (bov << 16) | (bmm << 24);
  return r;
}

// ---- the kernel's walk, lane by lane ----
static uint32_t sim_quality(const Bytes& q, uint32_t la, uint32_t cutoff, uint32_t W) {
  if (cutoff == 0) return la;
  int32_t carry = 0;
  bool stopped = false;
  TrmLow low[64];
  for (uint32_t lane = 0; lane < 64; ++lane) low[lane] = trm_low_none(la);
  for (int r = (int)W / 2 - 1; r >= 0; --r) {
    int32_t incl[64], next[64];
    bool in[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t t = 64u * (uint32_t)r + lane;
      in[lane] = t < la;
      incl[lane] = in[lane] ? trm_term(q[t], cutoff) : 0;
    }
    for (uint32_t o = 1; o < 64; o <<= 1) {
      for (uint32_t lane = 0; lane < 64; ++lane) next[lane] = trm_scan_add(incl[lane], incl[lane + o < 64 ? lane + o : lane], lane, o);
      memcpy(incl, next, sizeof(incl));
    }
    uint64_t pos = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) pos |= (uint64_t)(in[lane] & (carry + incl[lane] > 0)) << lane;
    const int32_t stop = trm_stop_lane(pos);
    int32_t want = -1;
    for (int b = 63; b >= 0 && want < 0; --b)
      if ((pos >> b) & 1) want = b;
    CHECK(stop == want);
    for (uint32_t lane = 0; lane < 64; ++lane)
      low[lane] = trm_low_take(low[lane], carry + incl[lane], 64u * (uint32_t)r + lane, in[lane] & !stopped & ((int32_t)lane > stop));
    stopped |= pos != 0;
    carry += incl[0];
  }
  for (int step = 32; step >= 1; step >>= 1) {
    TrmLow next[64];
    for (uint32_t lane = 0; lane < 64; ++lane) next[lane] = trm_low_combine(low[lane], low[lane ^ (uint32_t)step]);
    memcpy(low, next, sizeof(low));
  }
  for (uint32_t lane = 1; lane < 64; ++lane) CHECK(low[lane].s == low[0].s && low[lane].i == low[0].i);
  return trm_quality_len(low[0], la);
}

template <int P, bool IUPAC>
static TrmRecord sim_trim(const Bytes& a, const Bytes& q, const std::vector<Bytes>& ads, const Params& p, uint32_t W) {
  const uint32_t profile = IUPAC ? kHamIupac : kHamDna, la = (uint32_t)a.size(), S = W + kTrmPad;
  CHECK(la <= 32 * W);
  const uint32_t lq = sim_quality(q, la, p.cutoff, W);
  CHECK(lq <= la);
  // the planes in a buffer of exactly the kernel's size: a word read beyond it is the sanitizer's to report
  std::vector<uint32_t> planes((size_t)(P + 1) * S);
  trm_encode_read(profile, a.data(), la, lq, W, planes.data());
  std::vector<uint32_t> tab(std::max<size_t>(ads.size(), 1) * kTrmTableWords);
  for (size_t j = 0; j < ads.size(); ++j) trm_encode_adapter(profile, ads[j].data(), (uint32_t)ads[j].size(), tab.data() + j * kTrmTableWords);
  const uint32_t count = trm_positions(lq, p.min_overlap);
  TrmBest best[64];
  for (uint32_t lane = 0; lane < 64; ++lane) best[lane] = trm_none();
  for (uint32_t round = 0; round < ovl_rounds(count); ++round) {
    bool any = false;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t c_mine = round * kOvlWave + lane;
      const bool in_range = c_mine < count;
      const uint32_t c = in_range ? c_mine : count - 1u;
      CHECK((c >> 5) + 2 < S);
      uint32_t rw[P + 1][2];
      for (int pl = 0; pl <= P; ++pl) trm_window(planes.data() + (size_t)pl * S, c, rw[pl]);
      for (uint32_t j = 0; j < ads.size(); ++j) {
        const uint32_t* ad = tab.data() + j * kTrmTableWords;
        const uint32_t mm = trm_mismatches<P, IUPAC>(rw, ad), ov = trm_overlap(ad[kTrmLenWord], lq, c);
        best[lane] = trm_combine(best[lane], trm_one(c, ov, mm, j, in_range & ovl_accepts(mm, ov, p.min_overlap, p.k, p.max_permille)));
      }
      any |= best[lane].found != 0;
    }
    if (any) break;
  }
  for (int step = 32; step >= 1; step >>= 1) {
    TrmBest next[64];
    for (uint32_t lane = 0; lane < 64; ++lane) next[lane] = trm_combine(best[lane], best[lane ^ (uint32_t)step]);
    memcpy(best, next, sizeof(best));
  }
  for (uint32_t lane = 1; lane < 64; ++lane) CHECK(memcmp(&best[lane], &best[0], sizeof(TrmBest)) == 0);
  return trm_record(best[0], lq, p.min_length);
}

static TrmRecord sim(uint32_t profile, const Bytes& a, const Bytes& q, const std::vector<Bytes>& ads, const Params& p, uint32_t W) {
  return profile == kHamIupac ? sim_trim<4, true>(a, q, ads, p, W) : sim_trim<2, false>(a, q, ads, p, W);
}

static const uint32_t kAdapterLens[] = {1, 31, 32, 33, 63, 64};
static std::vector<uint32_t> read_lengths() {
  std::vector<uint32_t> v;
  for (uint32_t l = 0; l <= 130; ++l) v.push_back(l);
  for (uint32_t l : {191u, 192u, 193u, 255u, 256u, 257u, 511u, 512u}) v.push_back(l);
  return v;
}

static void check_one(uint32_t profile, uint32_t la, uint32_t m, uint32_t W, int planted_at) {
  Bytes a(la), q(la);
  for (auto& c : a) c = random_base(profile);
  const uint32_t cutoff = below(2) ? 0u : (uint32_t)(5 + below(30));
  for (uint32_t t = 0; t < la; ++t) q[t] = (uint8_t)(33 + below(42) / (1 + 3 * t / (la + 1)));  // decays toward the 3' end
  std::vector<Bytes> ads(1 + below(3));
  const size_t mine = below(ads.size());
  uint32_t shortest = m;
  for (size_t j = 0; j < ads.size(); ++j) {
    ads[j].resize(j == mine ? m : kAdapterLens[below(6)]);
    for (auto& c : ads[j]) c = random_base(profile);
    shortest = std::min(shortest, (uint32_t)ads[j].size());
  }
  if (ads.size() > 1 && below(4) == 0) ads[(mine + 1) % ads.size()] = ads[mine];  // a full tie: the smaller j
  if (planted_at >= 0) {
    for (uint32_t i = 0; i < m && (uint32_t)planted_at + i < la; ++i) a[(uint32_t)planted_at + i] = ads[mine][i];
    for (uint32_t e = below(3); e > 0; --e) a[below(la)] = random_base(profile);
  }
  const uint32_t ks[] = {0, 1, 2, 64}, pms[] = {0, 100, 250, 1000};
  const Params p{1 + (uint32_t)below(std::min(shortest, 6u)), ks[below(4)], pms[below(4)], cutoff, (uint32_t)below(la + 2)};
  const TrmRecord got = sim(profile, a, q, ads, p, W), want = brute_trim(profile, a, q, ads, p);
  if (memcmp(&got, &want, sizeof(got)) != 0) {
    fprintf(stderr, "profile %u la %u m %u W %u planted %d: got (%u %u %u %08x), want (%u %u %u %08x)\n", profile, la, m, W, planted_at, got.length,
            got.quality_len, got.adapter_pos, got.tail, want.length, want.quality_len, want.adapter_pos, want.tail);
    exit(1);
  }
}

static uint64_t check_refusals() {
  static const uint8_t ad0[4] = {'A', 'C', 'G', 'T'};
  const uint8_t* good[2] = {ad0, ad0};
  const uint8_t* with_null[2] = {ad0, nullptr};
  size_t lens[2] = {4, 4}, zero[2] = {4, 0}, longer[2] = {4, 65}, shorter[2] = {4, 2};
  // everything wrong at once; each step mends what was reported and expects the next in the order
  TrmCall c{};
  c.have_searcher = false; c.flags = 1; c.min_overlap = 0; c.max_permille = 1001; c.quality_cutoff = 94;
  c.adapters = nullptr; c.adapter_lens = nullptr; c.n_adapters = 65;
  c.gate.handles = 1;
  c.gate.profile = 0; c.gate.overhang = c.gate.only_best = c.gate.max_n_frac = true;
  c.gate.have_reads[0] = false; c.gate.handle_read = true; c.gate.device_s = 0; c.gate.device_r[0] = 1; c.gate.longest[0] = 513; c.kept_quality = false;
  c.have_trimmed = false; c.gate.in_flight = true;
  size_t which = 9;
  ReadsRefusal gate = kRdsOk;
  uint64_t n = 0;
  // (the call's own code, the gate's code, the adapter named)
#define EXPECT(code, gate_code, j) do { CHECK(trm_refusal(c, &which, &gate) == (code)); CHECK(gate == (gate_code) && which == (size_t)(j)); ++n; } while (0)
  EXPECT(kTrmNullSearcher, kRdsOk, 0); c.have_searcher = true;
  EXPECT(kTrmFlags, kRdsOk, 0); c.flags = 0;
  EXPECT(kTrmMinOverlap, kRdsOk, 0); c.min_overlap = 3;
  EXPECT(kTrmPermille, kRdsOk, 0); c.max_permille = 1000;
  EXPECT(kTrmCutoff, kRdsOk, 0); c.quality_cutoff = 93;
  EXPECT(kTrmTooMany, kRdsOk, 0); c.n_adapters = 2;
  EXPECT(kTrmNullAdapter, kRdsOk, 0); c.adapters = with_null; c.adapter_lens = lens;
  EXPECT(kTrmNullAdapter, kRdsOk, 1); c.adapters = good; c.adapter_lens = zero;
  EXPECT(kTrmEmptyAdapter, kRdsOk, 1); c.adapter_lens = longer;
  EXPECT(kTrmLongAdapter, kRdsOk, 1); c.adapter_lens = shorter;
  EXPECT(kTrmShortAdapter, kRdsOk, 1); c.adapter_lens = lens;
  EXPECT(kTrmGate, kRdsAscii, 0); c.gate.profile = kHamIupac;
  EXPECT(kTrmGate, kRdsOverhang, 0); c.gate.overhang = false;
  EXPECT(kTrmGate, kRdsOnlyBest, 0); c.gate.only_best = false;
  EXPECT(kTrmGate, kRdsNFrac, 0); c.gate.max_n_frac = false;
  EXPECT(kTrmGate, kRdsNullReads, 0); c.gate.have_reads[0] = true;
  EXPECT(kTrmGate, kRdsDevice, 0); c.gate.device_r[0] = 0;
  EXPECT(kTrmGate, kRdsTooLong, 0); c.gate.longest[0] = 512;
  EXPECT(kTrmNoQuality, kRdsOk, 0); c.quality_cutoff = 0;
  EXPECT(kTrmNullTrimmed, kRdsOk, 0); c.quality_cutoff = 20; c.kept_quality = true;
  EXPECT(kTrmNullTrimmed, kRdsOk, 0); c.have_trimmed = true;
  EXPECT(kTrmGate, kRdsInFlight, 0); c.gate.in_flight = false;
  EXPECT(kTrmOk, kRdsOk, 0);
  c.n_adapters = 0; c.adapters = nullptr; c.adapter_lens = nullptr;  // no adapter at all is a call
  EXPECT(kTrmOk, kRdsOk, 0);
  c.gate.handle_read = false; c.gate.longest[0] = 9999;  // before the handle is read nothing of it is judged
  EXPECT(kTrmOk, kRdsOk, 0);
#undef EXPECT
  return n;
}

static uint64_t check_blocks() {
  uint64_t blocks = 0;
  const uint32_t lens[] = {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200};
  for (uint32_t begin = 0; begin < 34; ++begin)
    for (uint32_t len : lens)
      for (uint32_t tail : {0u, 5u})
        for (uint64_t start : {0ull, 128ull}) {
          const uint32_t have = begin + len + tail;
          const uint64_t bytes = ((start + have + 63) & ~63ull) + (tail ? 64 : 0);  // (tail == 0: the read ends the buffer, no spare block)
          Bytes buf(bytes);  // exactly `bytes`: a piece that reaches beyond is the sanitizer's to report
          for (auto& c : buf) c = (uint8_t)(1 + below(255));  // garbage everywhere, the pads included
          const auto load16 = [&](uint64_t at, uint32_t* w) {
            CHECK(at % 16 == 0 && at + 16 <= bytes);
            memcpy(w, buf.data() + at, 16);
          };
          for (uint32_t pb = 0; pb < ((len + 63) & ~63u); pb += 64) {
            const uint32_t left = ham_rem(pb / 64, 0, len);
            CHECK(left == len - pb);
            uint32_t out[16];
            trm_window_block(load16, start + begin + pb, bytes, std::min(left, 64u), out);
            uint8_t got[64];
            memcpy(got, out, 64);
            for (uint32_t i = 0; i < 64; ++i) CHECK(got[i] == (pb + i < len ? buf[start + begin + pb + i] : 0));
            if (begin % 16 == 0) {  // the trim's path (begin == 0 there): the same block out of four aligned pieces
              for (uint32_t q = 0; q < 4; ++q) {
                uint32_t w[4];
                trm_aligned_quarter(load16, start + begin + pb, bytes, std::min(left, 64u), q, w);
                CHECK(memcmp(w, got + 16 * q, 16) == 0);
              }
            }
            ++blocks;
          }
        }
  return blocks;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  uint64_t reads = 0, positions = 0, walks = 0;
  const std::vector<uint32_t> lengths = read_lengths();
  for (uint32_t profile : {kHamDna, kHamIupac})
    for (uint32_t la : lengths)
      for (uint32_t m : kAdapterLens)
        for (uint32_t W : {ovl_words(la), kOvlMaxWords}) {
          check_one(profile, la, m, W, -1);
          ++reads;
          for (uint32_t c = 0; c < la; ++c, ++positions) check_one(profile, la, m, W, (int)c);
        }
  for (uint32_t la : lengths)
    for (uint32_t W : {ovl_words(la), kOvlMaxWords})
      for (int kind = 0; kind < 7; ++kind, ++walks) {
        const uint32_t cutoff = 1 + (uint32_t)below(93);
        Bytes q(la);
        for (auto& c : q) c = kind == 0 ? 33 : kind == 1 ? 126 : kind == 2 ? (uint8_t)(33 + cutoff) : kind == 3 ? (uint8_t)below(256) : (uint8_t)(33 + cutoff - 2 + below(5));
        CHECK(sim_quality(q, la, cutoff, W) == brute_quality(q, cutoff));
        if (kind == 0) CHECK(brute_quality(q, cutoff) == 0);
        if (kind == 1 && cutoff < 93) CHECK(brute_quality(q, cutoff) == la);
        if (kind == 2) CHECK(brute_quality(q, cutoff) == la);
      }
  const uint64_t refusals = check_refusals(), blocks = check_blocks();
  printf("ok reads=%llu positions=%llu walks=%llu refusals=%llu blocks=%llu\n", (unsigned long long)reads, (unsigned long long)positions,
         (unsigned long long)walks, (unsigned long long)refusals, (unsigned long long)blocks);
  return 0;
}
