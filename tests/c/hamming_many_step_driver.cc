// hamming_many_step_driver.cc -- drives what sassy_amd/csrc/hamming_step.h adds for a batch of texts, on the host against
// brute force: the per-text position mask (ham_rem, ham_valid_mask_rem), the block-to-text lookup (ham_text_of) over start
// tables with empty texts first, last and in runs, and the min-cost narrowing (ham_min_cost) over random counter planes.
// Built by tests/test_hamming_many_cpu.py with -fsanitize=address,undefined.
//   hamming_many_step_driver <seed>   prints "ok masks=<n> lookups=<n> minima=<n>", exit status 0; a mismatch: stderr, 1
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../sassy_amd/csrc/hamming_step.h"

using namespace sassy_hip;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static int fail(const std::string& what) {
  fprintf(stderr, "MISMATCH %s\n", what.c_str());
  return 1;
}

// ---- the position mask: start i of a block is kept iff i + m <= rem ----
static int check_masks(uint64_t* n) {
  const uint32_t ms[] = {1, 2, 63, 64, 65, 1024};
  for (uint32_t m : ms) {
    const uint64_t rems[] = {0, 1, (uint64_t)m - 1, m, (uint64_t)m + 1, 63, 64, 65, (uint64_t)m + 63, (uint64_t)m + 64, 0xFFFFFFFFull};
    for (uint64_t rem : rems) {
      uint64_t want = 0;
      for (uint32_t i = 0; i < 64; ++i)
        if ((uint64_t)i + m <= rem) want |= (uint64_t)1 << i;
      if (ham_valid_mask_rem((uint32_t)rem, m) != want) return fail("valid mask m=" + std::to_string(m) + " rem=" + std::to_string(rem));
      ++*n;
    }
  }
  // ham_rem: the bytes from a block's first byte to its text's end, saturated; and the two rules agree with the single-text
  // mask when the text is the whole buffer
  const uint64_t lens[] = {0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 0x100000000ull, 0x100000040ull + 7};
  for (uint64_t start : {(uint64_t)0, (uint64_t)64, (uint64_t)4096, (uint64_t)1 << 33})
    for (uint64_t len : lens)
      for (uint64_t b = start / 64; b < start / 64 + 3 + (len < 10000 ? len / 64 : 0); ++b) {
        const uint64_t end = start + len, s0 = b * 64;
        const uint64_t left = end > s0 ? end - s0 : 0;
        const uint32_t want = left > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)left;
        if (ham_rem(b, start, len) != want) return fail("rem start=" + std::to_string(start) + " len=" + std::to_string(len));
        for (uint32_t m : ms)
          if (ham_valid_mask_rem(ham_rem(b, start, len), m) != ham_valid_mask(b - start / 64, len, m))
            return fail("rem mask against the single-text mask, len=" + std::to_string(len) + " m=" + std::to_string(m));
        ++*n;
      }
  return 0;
}

// ---- the lookup: texts laid out from multiples of 64 on, an empty text takes no block ----
static int check_lookup(const std::vector<uint64_t>& lens, uint64_t* n) {
  std::vector<uint64_t> start;
  uint64_t total = 0;
  for (uint64_t l : lens) {
    start.push_back(total);
    total += (l + 63) / 64 * 64;
  }
  const uint32_t nt = (uint32_t)lens.size();
  auto at = [&](uint32_t i) { return start.at(i); };  // (.at: a read outside the table aborts)
  for (uint64_t b = 0; b < total / 64; ++b) {
    uint32_t want = nt;  // brute force: the text whose blocks hold block b
    for (uint32_t t = 0; t < nt; ++t)
      if (lens[t] && start[t] <= b * 64 && b * 64 < start[t] + (lens[t] + 63) / 64 * 64) want = t;
    if (want == nt) return fail("a block without a text");
    for (uint64_t pos : {b * 64, b * 64 + 63}) {
      const uint32_t got = ham_text_of(at, nt, pos);
      if (got != want || lens[got] == 0) return fail("lookup block " + std::to_string(b) + ": " + std::to_string(got) + " != " + std::to_string(want));
      ++*n;
    }
    // rem of the block through the lookup: what the device builds
    const uint32_t t = ham_text_of(at, nt, b * 64);
    const uint64_t left = start[t] + lens[t] - b * 64;
    if (ham_rem(b, start[t], lens[t]) != left || left == 0) return fail("rem through the lookup");
  }
  return 0;
}

// ---- the narrowing: minimum and who attains it, against the per-start counts ----
template <int P>
static int check_min(uint64_t* n) {
  for (int round = 0; round < 400; ++round) {
    HamCounter<P> cnt;
    for (int p = 0; p < P; ++p) cnt.c[p] = rnd();
    if (round % 4 == 1)  // few distinct counts: ties
      for (int p = 1; p < P; ++p) cnt.c[p] = (rnd() & 1) ? ~(uint64_t)0 : 0;
    cnt.over = round % 5 == 0 ? rnd() : round % 5 == 1 ? ~(uint64_t)0 : round % 5 == 2 ? rnd() & rnd() & rnd() : 0;
    uint32_t count[64];
    for (int i = 0; i < 64; ++i) {
      count[i] = 0;
      for (int p = 0; p < P; ++p) count[i] |= (uint32_t)((cnt.c[p] >> i) & 1u) << p;
    }
    std::vector<uint64_t> hits = {0, (uint64_t)1 << (rnd() & 63), ~(uint64_t)0, rnd(), rnd() & rnd(), 1, (uint64_t)1 << 63};
    // the minimum attained at bit 0 / at bit 63 only: clear that start's planes, raise the others' lowest plane
    for (int where : {0, 63}) {
      HamCounter<P> c2 = cnt;
      for (int p = 0; p < P; ++p) c2.c[p] &= ~((uint64_t)1 << where);
      c2.c[0] |= ~((uint64_t)1 << where);
      c2.over = 0;
      uint64_t at = 0;
      const uint32_t got = ham_min_cost<P>(c2, ~(uint64_t)0, &at);
      if (got != 0 || at != (uint64_t)1 << where) return fail("minimum at bit " + std::to_string(where));
      ++*n;
    }
    for (uint64_t hit : hits) {
      const uint64_t live = hit & ~cnt.over;
      uint32_t want = 0xFFFFFFFFu;
      uint64_t who = 0;
      for (int i = 0; i < 64; ++i)
        if ((live >> i) & 1u) {
          if (count[i] < want) { want = count[i]; who = 0; }
          if (count[i] == want) who |= (uint64_t)1 << i;
        }
      uint64_t at = ~(uint64_t)0;
      const uint32_t got = ham_min_cost<P>(cnt, hit, &at);
      if (got != want || at != who) return fail("narrowing P=" + std::to_string(P) + " round " + std::to_string(round));
      ++*n;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  uint64_t masks = 0, lookups = 0, minima = 0;
  if (check_masks(&masks)) return 1;
  const std::vector<std::vector<uint64_t>> tables = {
      {5},
      {0, 5},
      {0, 0, 0, 70, 1},
      {64, 0},
      {64, 0, 0, 0},
      {1, 0, 0, 128, 0, 129, 0, 0},
      {0, 0, 63, 0, 0, 64, 0, 0, 65, 0, 0},
      {4097, 0, 4096, 0, 4095},
  };
  for (const auto& t : tables)
    if (check_lookup(t, &lookups)) return 1;
  for (int round = 0; round < 50; ++round) {  // random tables, a third of the texts empty
    std::vector<uint64_t> lens;
    const uint32_t nt = 1 + (uint32_t)(rnd() % 40);
    for (uint32_t i = 0; i < nt; ++i) lens.push_back(rnd() % 3 == 0 ? 0 : rnd() % 300);
    bool any = false;
    for (uint64_t l : lens) any = any || l;
    if (!any) lens.back() = 1;
    if (check_lookup(lens, &lookups)) return 1;
  }
  if (check_min<2>(&minima) || check_min<4>(&minima) || check_min<8>(&minima) || check_min<11>(&minima)) return 1;
  printf("ok masks=%llu lookups=%llu minima=%llu\n", (unsigned long long)masks, (unsigned long long)lookups, (unsigned long long)minima);
  return 0;
}
