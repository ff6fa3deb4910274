// edit_pairs_step_driver.cc -- drives sassy_amd/csrc/edit_pairs_step.h (the arithmetic of sassy_hip_edit_pairs / _nearest,
// free of HIP) on the host: the entry planes, the packed record codes and the bit-vector column step against a plain
// byte-wise DP over ham_match, for every profile and every (m_a, m_b) in {1, 2, 31, 32, 33, 63, 64}^2 -- random pairs, equal
// pairs (the shorter a prefix of the longer where the lengths differ: E = |m_a - m_b|), pairs with no matching row
// (E = max(m_a, m_b)) and y = x shifted by one row, where every diagonal run crosses the word border at row 32.  Built by
// tests/test_edit_pairs_cpu.py with -fsanitize=address,undefined.
//   edit_pairs_step_driver <seed>   prints "ok random=<n> equal=<n> nomatch=<n> shifted=<n> codes=<n>", exit status 0;
//                                   a failed check: its line on stderr, 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sassy_amd/csrc/edit_pairs_step.h"

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
static const uint32_t kLengths[7] = {1, 2, 31, 32, 33, 63, 64};

static uint8_t random_byte(uint32_t profile) {
  static const char iupac[] = "ACGTUNRYSWKMBDHVacgtnry";
  static const char dna[] = "ACGTacgt";
  if (profile == kHamIupac) return (uint8_t)iupac[below(sizeof(iupac) - 1)];
  if (profile == kHamDna) return below(16) ? (uint8_t)dna[below(sizeof(dna) - 1)] : (uint8_t)below(256);
  return below(8) ? (uint8_t)("AaBb"[below(4)]) : (uint8_t)below(256);
}
// two bytes of the profile that do not match, whichever way round
static void disjoint_bytes(uint32_t profile, uint8_t* x, uint8_t* y) {
  *x = profile == kHamDna || profile == kHamIupac ? 'A' : 'q';
  *y = profile == kHamDna || profile == kHamIupac ? 'C' : 'Z';
  CHECK(!ham_match(profile, *x, *y) && !ham_match(profile, *y, *x));
}

// D[m_a][m_b] of the definition, two rows at a time
static uint32_t plain_dp(uint32_t profile, const std::vector<uint8_t>& x, const std::vector<uint8_t>& y) {
  const size_t m_a = x.size(), m_b = y.size();
  std::vector<uint32_t> col(m_a + 1), next(m_a + 1);
  for (size_t i = 0; i <= m_a; ++i) col[i] = (uint32_t)i;
  for (size_t j = 1; j <= m_b; ++j) {
    next[0] = (uint32_t)j;
    for (size_t i = 1; i <= m_a; ++i) {
      const uint32_t sub = col[i - 1] + (ham_match(profile, x[i - 1], y[j - 1]) ? 0u : 1u);
      next[i] = std::min(sub, std::min(col[i], next[i - 1]) + 1u);
    }
    col.swap(next);
  }
  return col[m_a];
}

static uint32_t cost_instantiated(uint32_t profile, uint32_t W, const uint32_t* a, const uint32_t* rec, uint32_t m_a, uint32_t m_b) {
  if (profile == kHamDna) return W == 1 ? edit_cost<2, 1, false>(a, rec, m_a, m_b) : edit_cost<2, 2, false>(a, rec, m_a, m_b);
  if (profile == kHamIupac) return W == 1 ? edit_cost<4, 1, true>(a, rec, m_a, m_b) : edit_cost<4, 2, true>(a, rec, m_a, m_b);
  return W == 1 ? edit_cost<8, 1, false>(a, rec, m_a, m_b) : edit_cost<8, 2, false>(a, rec, m_a, m_b);
}

static uint64_t n_codes = 0;
// E(x, y) as the kernel computes it, both ways round, against the plain DP; returns it
static uint32_t check_pair(uint32_t profile, const std::vector<uint8_t>& x, const std::vector<uint8_t>& y) {
  const uint32_t P = pairs_planes(profile);
  const uint32_t want = plain_dp(profile, x, y);
  CHECK(want == plain_dp(profile, y, x));  // (the relation is symmetric)
  for (int turn = 0; turn < 2; ++turn) {
    const std::vector<uint8_t>& e = turn ? y : x;
    const std::vector<uint8_t>& t = turn ? x : y;
    const uint32_t m_a = (uint32_t)e.size(), m_b = (uint32_t)t.size(), W = pairs_words(m_a);
    CHECK(W <= 2 && m_a <= kEditMaxRows && m_b <= kEditMaxRows);
    std::vector<uint32_t> planes(P * 2), rec(edit_record_words(P, m_b));  // (heap blocks of the exact size: a read past the end is seen)
    pairs_encode(profile, e.data(), m_a, W, planes.data());
    edit_encode_record(profile, t.data(), m_b, rec.data());
    for (uint32_t j = 0; j < m_b; ++j, ++n_codes) CHECK(edit_record_code(P, rec.data(), j) == pairs_row_code(profile, t[j]));
    CHECK(cost_instantiated(profile, W, planes.data(), rec.data(), m_a, m_b) == want);
    if (W == 1) {  // the two-word instantiation gives the same: its higher words are zero
      pairs_encode(profile, e.data(), m_a, 2, planes.data());
      CHECK(cost_instantiated(profile, 2, planes.data(), rec.data(), m_a, m_b) == want);
    }
  }
  return want;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  uint64_t n_random = 0, n_equal = 0, n_nomatch = 0, n_shifted = 0;
  for (uint32_t profile : kProfiles)
    for (uint32_t m_a : kLengths)
      for (uint32_t m_b : kLengths) {
        const uint32_t longer = std::max(m_a, m_b), shorter = std::min(m_a, m_b);
        std::vector<uint8_t> x(m_a), y(m_b);
        for (int round = 0; round < 20; ++round, ++n_random) {
          // unrelated, and near copies with a row dropped here and there: every distance turns up
          for (auto& c : x) c = random_byte(profile);
          size_t from = 0;
          for (auto& c : y) {
            if (round % 2 && below(12) == 0) ++from;
            c = round % 2 && from < m_a && below(10) ? x[from] : random_byte(profile);
            ++from;
          }
          const uint32_t e = check_pair(profile, x, y);
          CHECK(e >= longer - shorter && e <= longer);
        }
        for (int round = 0; round < 4; ++round, ++n_equal) {
          std::vector<uint8_t> z(longer);
          for (auto& c : z) c = random_byte(profile);
          std::copy(z.begin(), z.begin() + m_a, x.begin());
          std::copy(z.begin(), z.begin() + m_b, y.begin());
          CHECK(check_pair(profile, x, y) == longer - shorter);
        }
        for (int round = 0; round < 2; ++round, ++n_nomatch) {
          uint8_t cx, cy;
          disjoint_bytes(profile, &cx, &cy);
          std::fill(x.begin(), x.end(), round ? cy : cx);
          std::fill(y.begin(), y.end(), round ? cx : cy);
          CHECK(check_pair(profile, x, y) == longer);
        }
        for (int round = 0; round < 4; ++round, ++n_shifted) {
          // y[j] = x[j + 1] (rounds 0, 1) or x[j - 1] (2, 3): one deletion at one end, what the other end lacks made up
          for (auto& c : x) c = random_byte(profile);
          for (uint32_t j = 0; j < m_b; ++j) {
            const int64_t src = round < 2 ? (int64_t)j + 1 : (int64_t)j - 1;
            y[j] = src >= 0 && src < (int64_t)m_a ? x[(size_t)src] : random_byte(profile);
          }
          const uint32_t e = check_pair(profile, x, y);
          if (m_a == m_b) CHECK(e <= 2);
        }
      }
  printf("ok random=%llu equal=%llu nomatch=%llu shifted=%llu codes=%llu\n", (unsigned long long)n_random, (unsigned long long)n_equal,
         (unsigned long long)n_nomatch, (unsigned long long)n_shifted, (unsigned long long)n_codes);
  return 0;
}
