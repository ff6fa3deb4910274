// amplicon_step_driver.cc -- drives sassy_amd/csrc/amplicon_step.h on the host against brute force over bit arrays: the
// partner window, the lower bound on blocks inside a run of items, the count of a run's starts inside [lo, hi] (partial first
// and last mask, whole masks through the prefix, absent blocks), the j-th such start (first, last, out of range), and the
// ownership of a left hit by overlapping ranges of tiles.  Built by tests/test_amplicons_cpu.py with
// -fsanitize=address,undefined.
//   amplicon_step_driver <seed>   prints "ok windows=<n> bounds=<n> counts=<n> selects=<n> owners=<n>", exit status 0; a
//                                 mismatch: stderr, 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../sassy_amd/csrc/amplicon_step.h"

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

struct Item {
  uint64_t block, mask;
};

// A sorted list of items as the scan leaves it: the runs of several patterns one behind the other, each from a bit array with
// missing blocks; the prefix runs over the whole list.
struct List {
  std::vector<Item> items;
  std::vector<uint32_t> prefix;            // items.size() + 1
  std::vector<uint32_t> run;               // patterns + 1: pattern p owns items [run[p], run[p + 1])
  std::vector<std::vector<uint8_t>> bits;  // per pattern: the bit array, one byte per start
};

static List make_list(uint32_t patterns, uint32_t blocks, int style) {
  List l;
  l.run.push_back(0);
  for (uint32_t p = 0; p < patterns; ++p) {
    std::vector<uint8_t> bits((size_t)blocks * 64, 0);
    for (uint32_t b = 0; b < blocks; ++b) {
      uint64_t m = 0;
      switch ((style + (int)p) % 4) {
        case 0: m = rnd() & rnd(); break;                                  // a quarter of the starts
        case 1: m = (rnd() % 3 == 0) ? rnd() & rnd() & rnd() & rnd() : 0; break;  // sparse, most blocks missing
        case 2: m = (rnd() % 4 == 0) ? 0 : ~(uint64_t)0; break;            // dense, a block missing now and then
        default: m = (rnd() & 1) ? ((uint64_t)1 << 63) | 1u : 0; break;    // bit 0 and bit 63 only
      }
      if (m == 0) continue;
      l.items.push_back(Item{b, m});
      for (int i = 0; i < 64; ++i) bits[(size_t)b * 64 + i] = (uint8_t)((m >> i) & 1u);
    }
    l.run.push_back((uint32_t)l.items.size());
    l.bits.push_back(bits);
  }
  uint32_t hits = 0;
  for (const Item& it : l.items) {
    l.prefix.push_back(hits);
    hits += amp_popc(it.mask);
  }
  l.prefix.push_back(hits);
  return l;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  uint64_t windows = 0, bounds = 0, counts = 0, selects = 0, owners = 0;

  // ---- the partner window against the definition: every (p, L) ----
  for (int round = 0; round < 400; ++round) {
    const uint32_t a = 1 + rnd() % 40, b = 1 + rnd() % 40, bq = (rnd() & 1) ? a : b;
    const uint64_t min_len = 1 + rnd() % 60, max_len = rnd() % 5 == 0 ? min_len : min_len + rnd() % 60, s = rnd() % 300;
    uint64_t lo = 0, hi = 0;
    const bool some = amp_window(s, min_len, max_len, a, b, bq, &lo, &hi);
    bool any = false;
    for (uint64_t p = 0; p < 600; ++p) {
      const uint64_t end = p + bq;
      const bool in = end >= s && end - s >= min_len && end - s <= max_len && end - s >= a && end - s >= b;
      any = any || in;
      if (in != (some && p >= lo && p <= hi)) return fail("window s=" + std::to_string(s) + " p=" + std::to_string(p));
    }
    if (any != some) return fail("window emptiness");
    ++windows;
  }
  {  // a pair longer than max_len has no window; the shortest product of overlapping primers is max(a, b)
    uint64_t lo, hi;
    if (amp_window(5, 1, 19, 20, 18, 18, &lo, &hi)) return fail("window of a primer longer than max_len");
    if (!amp_window(5, 1, 20, 20, 18, 18, &lo, &hi) || lo != 7 || hi != 7) return fail("window of one start");
    windows += 2;
  }

  for (int round = 0; round < 60; ++round) {
    const uint32_t patterns = 1 + round % 4, blocks = 1 + (uint32_t)(rnd() % 12);
    const List l = make_list(patterns, blocks, round);
    auto block = [&](uint32_t i) { return l.items[i].block; };
    auto mask = [&](uint32_t i) { return l.items[i].mask; };
    auto prefix = [&](uint32_t i) { return l.prefix[i]; };
    const uint64_t n = (uint64_t)blocks * 64;
    for (uint32_t p = 0; p < patterns; ++p) {
      const uint32_t i0 = l.run[p], i1 = l.run[p + 1];
      // ---- the lower bound on blocks, inside the run only ----
      for (uint64_t b = 0; b <= blocks + 1; ++b) {
        uint32_t want = i0;
        while (want < i1 && l.items[want].block < b) ++want;
        if (amp_lower_bound(block, i0, i1, b) != want) return fail("lower bound b=" + std::to_string(b));
        ++bounds;
      }
      // ---- windows: ends on bit 0, bit 63 and one before and after each, empty ones, one start, random ones ----
      std::vector<std::pair<uint64_t, uint64_t>> wins;
      for (uint64_t b = 0; b < blocks; ++b)
        for (int64_t d : {-1, 0, 1, 62, 63, 64}) {
          const int64_t e = (int64_t)b * 64 + d;
          if (e < 0) continue;
          wins.push_back({(uint64_t)e, (uint64_t)e});                        // one start
          wins.push_back({(uint64_t)e, (uint64_t)e + rnd() % (n + 64)});     // lo on the edge
          wins.push_back({(uint64_t)e > 100 ? (uint64_t)e - rnd() % 100 : 0, (uint64_t)e});  // hi on the edge
          if (e > 0) wins.push_back({(uint64_t)e, (uint64_t)e - 1});         // empty: reversed
        }
      for (int i = 0; i < 40; ++i) {
        const uint64_t lo = rnd() % (n + 70);
        wins.push_back({lo, lo + rnd() % (n + 70)});
      }
      wins.push_back({0, n + 1000});
      wins.push_back({n, n + 1000});  // behind every item
      for (const auto& w : wins) {
        const uint64_t lo = w.first, hi = w.second;
        std::vector<uint64_t> want;
        for (uint64_t s = lo; s <= hi && s < n; ++s)
          if (l.bits[p][s]) want.push_back(s);
        if (amp_count(block, mask, prefix, i0, i1, lo, hi) != want.size())
          return fail("count lo=" + std::to_string(lo) + " hi=" + std::to_string(hi) + " round=" + std::to_string(round));
        ++counts;
        // ---- the j-th start: first, last, a few in between, out of range ----
        std::vector<uint64_t> js = {0, (uint64_t)want.size(), (uint64_t)want.size() + 1, (uint64_t)want.size() + 1000};
        if (!want.empty()) {
          js.push_back(want.size() - 1);
          for (int i = 0; i < 6; ++i) js.push_back(rnd() % want.size());
        }
        for (uint64_t j : js) {
          uint64_t got = ~(uint64_t)0;
          const bool ok = amp_select(block, mask, prefix, i0, i1, lo, hi, j, &got);
          if (ok != (j < want.size()) || (ok && got != want[j]))
            return fail("select lo=" + std::to_string(lo) + " hi=" + std::to_string(hi) + " j=" + std::to_string(j) + " round=" + std::to_string(round));
          ++selects;
        }
      }
      // one clipped item against its bits
      for (uint32_t i = i0; i < i1; ++i) {
        const uint64_t lo = rnd() % (n + 64), hi = lo + rnd() % 200;
        uint64_t want = 0;
        for (int bit = 0; bit < 64; ++bit) {
          const uint64_t s = l.items[i].block * 64 + bit;
          if (s >= lo && s <= hi && ((l.items[i].mask >> bit) & 1u)) want |= (uint64_t)1 << bit;
        }
        if (amp_clip(l.items[i].block, l.items[i].mask, lo, hi) != want) return fail("clip");
      }
    }
  }

  // ---- ownership: ranges that advance as the driver's do own every start exactly once, and only with all its partners ----
  for (int round = 0; round < 200; ++round) {
    const uint64_t max_len = 1 + rnd() % (3 * kAmpTileBytes), tiles = 1 + rnd() % 20, n = tiles * kAmpTileBytes;
    const uint64_t min_span = amp_min_span(max_len);
    std::vector<int> owned(n, 0);
    uint64_t own_from = 0, t0 = 0;
    for (int guard = 0;; ++guard) {
      if (guard > 10000) return fail("ranges do not advance");
      const uint64_t span = std::min<uint64_t>(tiles - t0, min_span + rnd() % 3), t1 = t0 + span;
      const bool last = t1 == tiles;
      for (uint64_t s = t0 * kAmpTileBytes; s < n && s < t1 * kAmpTileBytes + 10; ++s)
        if (amp_owns(s, own_from, t1, last, max_len)) {
          if (s < t0 * kAmpTileBytes) return fail("owned in front of the range");
          if (!last && s + max_len > t1 * kAmpTileBytes) return fail("owned without its partners");
          ++owned[s];
        }
      if (last) break;
      const uint64_t next = amp_next_from(own_from, t1, max_len);
      if (next / kAmpTileBytes <= t0) return fail("the next range does not begin behind this one's first tile");
      own_from = next;
      t0 = next / kAmpTileBytes;
    }
    for (uint64_t s = 0; s < n; ++s)
      if (owned[s] != 1) return fail("start " + std::to_string(s) + " owned " + std::to_string(owned[s]) + " times, max_len " + std::to_string(max_len));
    ++owners;
  }
  printf("ok windows=%llu bounds=%llu counts=%llu selects=%llu owners=%llu\n", (unsigned long long)windows, (unsigned long long)bounds,
         (unsigned long long)counts, (unsigned long long)selects, (unsigned long long)owners);
  return 0;
}
