// hamming_counts_step_driver.cc -- drives what sassy_amd/csrc/hamming_step.h adds for hamming_counts, on the host against
// brute force: HamCounter::eq over random counter planes (every count up to 2^P - 1, `over` set on some, none and all
// starts), the partition of le(k) into the eq(c), c <= k, and the min / max cost helpers that bound the wavefront's loop over
// costs, on the hit masks the narrowing driver uses.  Built by tests/test_hamming_counts_cpu.py with
// -fsanitize=address,undefined.
//   hamming_counts_step_driver <seed>   prints "ok eqs=<n> partitions=<n> bounds=<n> folds=<n>", exit status 0; a mismatch: stderr, 1
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

template <int P>
static void counts_of(const HamCounter<P>& cnt, uint32_t (&count)[64]) {
  for (int i = 0; i < 64; ++i) {
    count[i] = 0;
    for (int p = 0; p < P; ++p) count[i] |= (uint32_t)((cnt.c[p] >> i) & 1u) << p;
  }
}

template <int P>
static HamCounter<P> random_counter(int round) {
  HamCounter<P> cnt;
  for (int p = 0; p < P; ++p) cnt.c[p] = rnd();
  if (round % 4 == 1)  // few distinct counts
    for (int p = 1; p < P; ++p) cnt.c[p] = (rnd() & 1) ? ~(uint64_t)0 : 0;
  if (round % 4 == 2)  // small counts: the high planes mostly clear
    for (int p = P / 2; p < P; ++p) cnt.c[p] &= rnd() & rnd() & rnd();
  cnt.over = round % 5 == 0 ? rnd() : round % 5 == 1 ? ~(uint64_t)0 : round % 5 == 2 ? rnd() & rnd() & rnd() : 0;  // some / all / few / none
  return cnt;
}

// ---- eq(c) for every c < 2^P, and the partition of le(k) ----
template <int P>
static int check_eq(int rounds, uint64_t* eqs, uint64_t* partitions) {
  const uint32_t top = (1u << P) - 1u;
  for (int round = 0; round < rounds; ++round) {
    const HamCounter<P> cnt = random_counter<P>(round);
    uint32_t count[64];
    counts_of<P>(cnt, count);
    uint64_t seen = 0;  // OR of eq(0 .. c)
    for (uint32_t c = 0; c <= top; ++c) {
      uint64_t want = 0;
      for (int i = 0; i < 64; ++i)
        if (count[i] == c && !((cnt.over >> i) & 1u)) want |= (uint64_t)1 << i;
      const uint64_t got = cnt.eq(c);
      if (got != want) return fail("eq P=" + std::to_string(P) + " c=" + std::to_string(c) + " round " + std::to_string(round));
      if (got & seen) return fail("eq(c) overlaps a smaller cost, P=" + std::to_string(P));
      seen |= got;
      ++*eqs;
      if (seen != cnt.le(c)) return fail("OR of eq(0..k) != le(k), P=" + std::to_string(P) + " k=" + std::to_string(c));
      ++*partitions;
    }
    if (seen != ~cnt.over) return fail("the eq(c) do not cover the starts that are not saturated");
    if (cnt.le(top + 5) != seen) return fail("le beyond the planes");
  }
  return 0;
}

// ---- the bounds of the loop over costs: ham_min_cost / ham_max_cost ----
template <int P>
static int check_bounds(uint64_t* n, uint64_t* folds) {
  for (int round = 0; round < 400; ++round) {
    const HamCounter<P> cnt = random_counter<P>(round);
    uint32_t count[64];
    counts_of<P>(cnt, count);
    const std::vector<uint64_t> hits = {0, (uint64_t)1 << (rnd() & 63), ~(uint64_t)0, rnd(), rnd() & rnd(), 1, (uint64_t)1 << 63};
    // the extremes at bit 0 / at bit 63 only
    for (int where : {0, 63}) {
      HamCounter<P> lo = cnt, hi = cnt;
      for (int p = 0; p < P; ++p) {
        lo.c[p] &= ~((uint64_t)1 << where);
        hi.c[p] |= (uint64_t)1 << where;
      }
      lo.c[0] |= ~((uint64_t)1 << where);     // every other start: at least 1
      hi.c[0] &= (uint64_t)1 << where;        // every other start: below the top
      lo.over = hi.over = 0;
      uint64_t at = 0;
      if (ham_min_cost<P>(lo, ~(uint64_t)0, &at) != 0 || at != (uint64_t)1 << where) return fail("minimum at bit " + std::to_string(where));
      if (ham_max_cost<P>(hi, ~(uint64_t)0) != (1u << P) - 1u) return fail("maximum at bit " + std::to_string(where));
      if (ham_max_cost<P>(hi, ~((uint64_t)1 << where)) >= (1u << P) - 1u) return fail("maximum without bit " + std::to_string(where));
      *n += 3;
    }
    for (uint64_t hit : hits) {
      const uint64_t live = hit & ~cnt.over;
      uint32_t lo = 0xFFFFFFFFu, hi = 0;
      for (int i = 0; i < 64; ++i)
        if ((live >> i) & 1u) {
          if (count[i] < lo) lo = count[i];
          if (count[i] > hi) hi = count[i];
        }
      uint64_t at;
      const uint32_t got_lo = ham_min_cost<P>(cnt, hit, &at), got_hi = ham_max_cost<P>(cnt, hit);
      if (got_lo != lo || got_hi != hi) return fail("bounds P=" + std::to_string(P) + " round " + std::to_string(round));
      ++*n;
      // the fold as the kernel runs it: the popcounts of eq(c) & hit over c = lo .. hi add up to the hits, nothing lies outside
      if (live) {
        uint64_t sum = 0;
        for (uint32_t c = got_lo; c <= got_hi; ++c) {
          uint32_t want = 0;
          for (int i = 0; i < 64; ++i) want += ((live >> i) & 1u) && count[i] == c;
          const uint32_t got = (uint32_t)__builtin_popcountll(cnt.eq(c) & hit);
          if (got != want) return fail("fold P=" + std::to_string(P) + " c=" + std::to_string(c));
          sum += got;
        }
        if (sum != (uint64_t)__builtin_popcountll(live)) return fail("the fold loses hits, P=" + std::to_string(P));
        ++*folds;
      }
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  uint64_t eqs = 0, partitions = 0, bounds = 0, folds = 0;
  if (check_eq<2>(200, &eqs, &partitions) || check_eq<4>(200, &eqs, &partitions) || check_eq<8>(100, &eqs, &partitions) ||
      check_eq<11>(20, &eqs, &partitions))
    return 1;
  if (check_bounds<2>(&bounds, &folds) || check_bounds<4>(&bounds, &folds) || check_bounds<8>(&bounds, &folds) || check_bounds<11>(&bounds, &folds))
    return 1;
  printf("ok eqs=%llu partitions=%llu bounds=%llu folds=%llu\n", (unsigned long long)eqs, (unsigned long long)partitions,
         (unsigned long long)bounds, (unsigned long long)folds);
  return 0;
}
