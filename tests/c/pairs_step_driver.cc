// pairs_step_driver.cc -- drives sassy_amd/csrc/pairs_step.h (the arithmetic of sassy_hip_hamming_pairs / _nearest, free of
// HIP) on the host: the bit-plane encoding and the per-word distance against a byte-wise count of ham_match, every profile
// and the lengths around the word borders (the Iupac pad-bit rule included); the partial cells' combine rule against one
// sequential walk, for random splits; the plan -- every (i, j, strand) a call visits lies in exactly one walked tile, and no
// self-mode tile that holds a visited pair is skipped.  Built by tests/test_hamming_pairs_cpu.py with
// -fsanitize=address,undefined.
//   pairs_step_driver <seed>   prints "ok costs=<n> combines=<n> plans=<n> cells=<n>", exit status 0;
//                              a failed check: its line on stderr, 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sassy_amd/csrc/pairs_step.h"

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
static const uint32_t kProfiles[4] = {kHamDna, kHamIupac, kAscii, kHamAsciiCi};
static const uint32_t kLengths[10] = {1, 31, 32, 33, 63, 64, 65, 96, 127, 128};

static uint8_t random_byte(uint32_t profile) {
  static const char iupac[] = "ACGTUNRYSWKMBDHVXacgtnry";
  static const char dna[] = "ACGTacgtNn-*";
  if (profile == kHamIupac) return (uint8_t)iupac[below(sizeof(iupac) - 1)];
  if (profile == kHamDna) return below(8) ? (uint8_t)dna[below(sizeof(dna) - 1)] : (uint8_t)below(256);
  return below(4) ? (uint8_t)("AaBbZz@[`{"[below(10)]) : (uint8_t)below(256);
}

template <int P, int W, bool IUPAC>
static uint32_t cost_as_the_kernel(const uint32_t* a, const uint32_t* b, uint32_t m) { return pairs_cost<P, W, IUPAC>(a, b, m); }
static uint32_t cost_instantiated(uint32_t profile, uint32_t W, const uint32_t* a, const uint32_t* b, uint32_t m) {
  if (profile == kHamDna) return W == 1 ? cost_as_the_kernel<2, 1, false>(a, b, m) : W == 2 ? cost_as_the_kernel<2, 2, false>(a, b, m) : cost_as_the_kernel<2, 4, false>(a, b, m);
  if (profile == kHamIupac) return W == 1 ? cost_as_the_kernel<4, 1, true>(a, b, m) : W == 2 ? cost_as_the_kernel<4, 2, true>(a, b, m) : cost_as_the_kernel<4, 4, true>(a, b, m);
  return W == 1 ? cost_as_the_kernel<8, 1, false>(a, b, m) : W == 2 ? cost_as_the_kernel<8, 2, false>(a, b, m) : cost_as_the_kernel<8, 4, false>(a, b, m);
}

// encoding and per-word distance against the byte-wise count
static uint64_t check_costs() {
  uint64_t n = 0;
  for (uint32_t profile : kProfiles)
    for (uint32_t m : kLengths) {
      const uint32_t W = pairs_words(m), P = pairs_planes(profile);
      CHECK(W == 1 || W == 2 || W == 4);
      CHECK(32 * W >= m && P * W <= 32);
      for (int round = 0; round < 60; ++round) {
        std::vector<uint8_t> x(m), y(m);
        for (uint32_t t = 0; t < m; ++t) {
          x[t] = random_byte(profile);
          // near copies, full copies, unrelated: every distance from 0 to m turns up
          y[t] = round % 3 == 0 ? x[t] : (round % 3 == 1 && below(8)) ? x[t] : random_byte(profile);
        }
        if (round == 1 && profile == kHamIupac) {  // all N: every row matches, the pad bits must not count
          std::fill(x.begin(), x.end(), (uint8_t)'N');
          std::fill(y.begin(), y.end(), (uint8_t)'N');
        }
        if (round == 2 && profile == kHamIupac) {  // disjoint sets on every row: cost m, the pad bits must not add to it
          std::fill(x.begin(), x.end(), (uint8_t)'A');
          std::fill(y.begin(), y.end(), (uint8_t)'C');
        }
        uint32_t want = 0;
        for (uint32_t t = 0; t < m; ++t) want += !ham_match(profile, x[t], y[t]);
        std::vector<uint32_t> ex(P * W), ey(P * W);
        pairs_encode(profile, x.data(), m, W, ex.data());
        pairs_encode(profile, y.data(), m, W, ey.data());
        // pad bits are zero in every plane
        for (uint32_t p = 0; p < P; ++p)
          for (uint32_t w = 0; w < W; ++w) CHECK((ex[p * W + w] & ~pairs_row_mask(m, w)) == 0);
        CHECK(cost_instantiated(profile, W, ex.data(), ey.data(), m) == want);
        CHECK(cost_instantiated(profile, W, ey.data(), ex.data(), m) == want);  // (symmetric)
        if (round == 1 && profile == kHamIupac) CHECK(want == 0);
        if (round == 2 && profile == kHamIupac) CHECK(want == m);
        if (W < 4) {  // a wider instantiation gives the same: its higher words are zero
          std::vector<uint32_t> wx(P * 4), wy(P * 4);
          pairs_encode(profile, x.data(), m, 4, wx.data());
          pairs_encode(profile, y.data(), m, 4, wy.data());
          CHECK(cost_instantiated(profile, 4, wx.data(), wy.data(), m) == want);
        }
        ++n;
      }
    }
  // the reverse complement helper reverses and complements
  const uint8_t seq[5] = {'A', 'C', 'G', 'T', 'N'};
  uint8_t out[5];
  pairs_reverse_complement(seq, 5, [](uint8_t c) { return c == 'A' ? (uint8_t)'T' : c == 'T' ? (uint8_t)'A' : c == 'C' ? (uint8_t)'G' : c == 'G' ? (uint8_t)'C' : c; }, out);
  CHECK(memcmp(out, "NACGT", 5) == 0);
  return n;
}

// the combine rule against one sequential walk
static uint64_t check_combines() {
  uint64_t n = 0;
  for (int round = 0; round < 2000; ++round) {
    const uint32_t len = (uint32_t)below(40), k = (uint32_t)below(6);
    std::vector<uint32_t> cost(len);
    for (uint32_t& c : cost) c = (uint32_t)below(9);
    // the walk: smallest (cost, r), ties at the final minimum, candidates
    uint32_t best = kPairsNoCost, best_r = 0xFFFFFFFFu, ties = 0, hits = 0;
    for (uint32_t r = 0; r < len; ++r)
      if (cost[r] <= k) {
        ++hits;
        if (cost[r] < best) { best = cost[r]; best_r = r; }
      }
    for (uint32_t r = 0; r < len; ++r) ties += cost[r] <= k && cost[r] == best;
    // random splits into runs, each run folded candidate by candidate, the runs folded in order
    PairsCell all = pairs_empty_cell();
    for (uint32_t r = 0; r < len;) {
      uint32_t end = r + (uint32_t)below(len - r + 1);
      if (end == r) {  // an empty run (a skipped tile) changes nothing
        all = pairs_combine(all, pairs_empty_cell());
        end = r + 1;
      }
      PairsCell run = pairs_empty_cell();
      for (; r < end; ++r)
        if (cost[r] <= k) run = pairs_combine(run, PairsCell{cost[r], r, 1u, 1u});
      all = pairs_combine(all, run);
    }
    CHECK(all.n_hits == hits && all.cost == best && all.ties == ties);
    CHECK(hits == 0 ? (all.r == 0xFFFFFFFFu && all.ties == 0) : all.r == best_r);
    ++n;
  }
  return n;
}

// the plan: every visited (i, j, strand) in exactly one walked tile
static uint64_t check_plans(uint64_t* cells) {
  static const uint64_t sizes[8] = {1, 63, 64, 65, 255, 256, 257, 1000};
  static const long forced[5] = {0, 1, 2, 3, 7};
  uint64_t n = 0;
  for (uint64_t n_a : sizes)
    for (uint64_t n_b : sizes)
      for (uint32_t mode : {kPairsCross, kPairsSelfPairs, kPairsSelfNearest})
        for (long f : forced) {
          if (mode != kPairsCross && n_b != n_a) continue;
          const PairsPlan p = pairs_plan(n_a, n_b, mode, f);
          CHECK(p.n_strips == (n_a + kPairsStrip - 1) / kPairsStrip);
          CHECK(p.n_chunks >= 1 && p.n_chunks <= kPairsMaxChunks && p.n_chunks <= n_b);
          if (f > 0) CHECK(p.n_chunks == (uint32_t)std::min<uint64_t>((uint64_t)f, n_b) || p.chunk * p.n_chunks >= n_b);
          CHECK(pairs_chunk_begin(p.chunk, 0) == 0 && pairs_chunk_end(p.chunk, n_b, p.n_chunks - 1) == n_b);
          std::vector<uint8_t> seen(n_a * n_b, 0);
          for (uint64_t i0 = 0; i0 < p.n_strips * kPairsStrip; i0 += kPairsWave)
            for (uint32_t c = 0; c < p.n_chunks; ++c) {
              const uint64_t j0 = pairs_chunk_begin(p.chunk, c), j1 = pairs_chunk_end(p.chunk, n_b, c);
              CHECK(j0 < j1);  // (no empty chunk)
              const uint64_t jf = pairs_tile_first(mode, i0, j0, j1);
              CHECK(j0 <= jf && jf <= j1);
              for (uint64_t i = i0; i < std::min(i0 + kPairsWave, n_a); ++i)
                for (uint64_t j = jf; j < j1; ++j) ++seen[i * n_b + j];
              *cells += 1;
            }
          for (uint64_t i = 0; i < n_a; ++i)
            for (uint64_t j = 0; j < n_b; ++j) {
              const bool wanted = pairs_visits(mode, i, j, 0) || pairs_visits(mode, i, j, 1);
              CHECK(seen[i * n_b + j] <= 1);
              if (wanted) CHECK(seen[i * n_b + j] == 1);
            }
          // self mode: strand 0 is j > i, strand 1 is j >= i; nearest leaves out (i, i, 0) alone
          if (mode == kPairsSelfPairs) CHECK(!pairs_visits(mode, 5, 5, 0) && pairs_visits(mode, 5, 5, 1) && pairs_visits(mode, 5, 6, 0) && !pairs_visits(mode, 6, 5, 1));
          if (mode == kPairsSelfNearest) CHECK(!pairs_visits(mode, 5, 5, 0) && pairs_visits(mode, 5, 5, 1) && pairs_visits(mode, 6, 5, 0));
          ++n;
        }
  // the planner's own choice: a small A gets chunks, a large A fills the device alone, the partials matrix stays bounded
  CHECK(pairs_plan(100, 4000000, kPairsCross, 0).n_chunks == 2048);
  CHECK(pairs_plan(1000000, 100000, kPairsCross, 0).n_chunks == 1);
  CHECK(pairs_plan(1000, 300, kPairsCross, 0).n_chunks == 1);
  CHECK(pairs_plan(5, 5, kPairsCross, 7).n_chunks == 5);
  CHECK((uint64_t)pairs_plan(1u << 20, 1u << 22, kPairsCross, 0).n_chunks * (1u << 20) <= (1ull << 24));
  // hamming_pairs asks for chunks of at most kPairsFineChunk targets, within the bound on the partials matrix
  CHECK(pairs_plan(100000, 100000, kPairsSelfPairs, 0, kPairsFineChunk).n_chunks == 7);
  CHECK(pairs_plan(1000000, 1000000, kPairsSelfPairs, 0, kPairsFineChunk).n_chunks == 16);
  CHECK(pairs_plan(100, 4000000, kPairsCross, 0, kPairsFineChunk).n_chunks == 2048);
  CHECK(pairs_plan(1000, 300, kPairsCross, 0, kPairsFineChunk).n_chunks == 1);
  CHECK(pairs_plan(10, 0x7FFFFFFFull, kPairsCross, 1u << 20).n_chunks <= kPairsMaxChunks);
  return n;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const uint64_t costs = check_costs();
  const uint64_t combines = check_combines();
  uint64_t cells = 0;
  const uint64_t plans = check_plans(&cells);
  printf("ok costs=%llu combines=%llu plans=%llu cells=%llu\n", (unsigned long long)costs, (unsigned long long)combines,
         (unsigned long long)plans, (unsigned long long)cells);
  return 0;
}
