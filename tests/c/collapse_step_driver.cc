// collapse_step_driver.cc -- drives sassy_amd/csrc/collapse_step.h (the duplicate table of sassy_hip_umi_groups, free of HIP)
// on the host, its memory policy instantiated with std::atomic.  Lists of up to 4000 keys -- all equal, all distinct, and
// mixtures with a few heavy classes -- are inserted into tables at the default size and at load 1 (one slot per entry, so the
// probes wrap round), with the real hash and with a hash forced to a constant (every probe sequence the same), and every
// entry's looked-up value is checked against a std::map from key to first index: the answer may not depend on the hash, the
// table's size or the order of the inserts.  Then the same inserts from up to 8 threads, dealt out in another order.
// Built by tests/test_umi_groups_cpu.py with -fsanitize=address,undefined and again with -fsanitize=thread.
//   collapse_step_driver <seed>   prints "ok tables=<n> inserts=<n> threaded=<n>", exit status 0;
//                                 a failed check: its line on stderr, 1
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <thread>
#include <vector>

#include "../../sassy_amd/csrc/collapse_step.h"

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
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

// the policy of collapse_step.h over std::atomic, relaxed
struct HostMem {
  std::atomic<uint32_t>* slots;
  uint32_t load(uint64_t x) const { return slots[x].load(std::memory_order_relaxed); }
  uint32_t cas(uint64_t x, uint32_t expect, uint32_t desired) const {
    (void)slots[x].compare_exchange_strong(expect, desired, std::memory_order_relaxed, std::memory_order_relaxed);
    return expect;
  }
  uint32_t fetch_min(uint64_t x, uint32_t value) const {
    uint32_t seen = slots[x].load(std::memory_order_relaxed);
    while (value < seen && !slots[x].compare_exchange_weak(seen, value, std::memory_order_relaxed, std::memory_order_relaxed)) {
    }
    return seen;
  }
};

constexpr uint32_t kWords = 2;  // words per key
typedef std::vector<uint32_t> Keys;  // [n][kWords]

// kind 0: all equal; 1: all distinct; 2: mixed -- a few heavy classes, many light ones, some singletons
static Keys make_keys(uint32_t kind, uint32_t n) {
  Keys keys((size_t)n * kWords);
  const uint32_t heavy = 1 + below(4), light = 1 + n / 8;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t cls;
    if (kind == 0) cls = 7;
    else if (kind == 1) cls = i;
    else cls = below(3) == 0 ? below(heavy) : below(2) ? 100 + below(light) : 1000000 + i;
    keys[(size_t)i * kWords] = cls * 2654435761u;
    keys[(size_t)i * kWords + 1] = cls ^ 0x5555AAAAu;
  }
  return keys;
}

struct Same {
  const Keys& keys;
  uint32_t i;
  bool operator()(uint32_t v) const { return std::equal(keys.begin() + (size_t)v * kWords, keys.begin() + (size_t)(v + 1) * kWords, keys.begin() + (size_t)i * kWords); }
};

// hash_kind 0: collapse_hash; 1: the constant 0; 2: a constant that starts the probes at the last slot
static uint32_t hash_of(const Keys& keys, uint32_t i, uint32_t hash_kind, uint64_t n_slots) {
  if (hash_kind == 1) return 0;
  if (hash_kind == 2) return (uint32_t)(n_slots - 1);
  return collapse_hash(keys.data() + (size_t)i * kWords, kWords);
}

static std::pair<uint32_t, uint32_t> key_of(const Keys& keys, uint32_t i) { return std::make_pair(keys[(size_t)i * kWords], keys[(size_t)i * kWords + 1]); }

static void check_table(HostMem& mem, const Keys& keys, uint32_t n, uint64_t n_slots, uint32_t hash_kind) {
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> first;
  for (uint32_t i = 0; i < n; ++i) first.insert(std::make_pair(key_of(keys, i), i));  // (the first insert of a key stays)
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t rep = collapse_lookup(mem, n_slots, hash_of(keys, i, hash_kind, n_slots), i, Same{keys, i});
    CHECK(rep == first[key_of(keys, i)]);
    CHECK(rep <= i);
  }
  // a class takes one slot: as many slots in use as there are keys, each holding a first index
  uint64_t used = 0;
  for (uint64_t q = 0; q < n_slots; ++q) {
    const uint32_t v = mem.load(q);
    if (v == kCollapseEmpty) continue;
    ++used;
    CHECK(v < n && first[key_of(keys, v)] == v);
  }
  CHECK(used == first.size());
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  static const uint32_t kSizes[] = {1, 2, 3, 64, 65, 257, 1000, 4000};
  uint64_t tables = 0, inserts = 0, threaded = 0;
  CHECK(collapse_slots_for(1, 0) == 2 && collapse_slots_for(1000, 0) == 2048 && collapse_slots_for(1024, 0) == 2048 && collapse_slots_for(1025, 0) == 4096);
  CHECK(collapse_slots_for(1000, 1000) == 1000 && collapse_slots_for(1000, 10) == 1000 && collapse_slots_for(1000, 1500) == 1500);
  for (uint32_t kind = 0; kind < 3; ++kind) {
    for (uint32_t n : kSizes) {
      const Keys keys = make_keys(kind, n);
      for (uint32_t geometry = 0; geometry < 2; ++geometry) {  // the default table, and load 1
        const uint64_t n_slots = collapse_slots_for(n, geometry ? (long)n : 0);
        CHECK(n_slots >= n);
        std::unique_ptr<std::atomic<uint32_t>[]> slots(new std::atomic<uint32_t>[n_slots]);
        HostMem mem{slots.get()};
        for (uint32_t hash_kind = 0; hash_kind < 3; ++hash_kind) {
          // one thread: ascending, descending or shuffled order
          std::vector<uint32_t> order(n);
          for (uint32_t i = 0; i < n; ++i) order[i] = i;
          const uint32_t how = below(3);
          if (how == 1) std::reverse(order.begin(), order.end());
          if (how == 2)
            for (size_t q = n; q > 1; --q) std::swap(order[q - 1], order[below((uint32_t)q)]);
          for (uint64_t q = 0; q < n_slots; ++q) slots[q].store(kCollapseEmpty, std::memory_order_relaxed);
          for (uint32_t i : order) {
            CHECK(collapse_insert(mem, n_slots, hash_of(keys, i, hash_kind, n_slots), i, Same{keys, i}));
            ++inserts;
          }
          check_table(mem, keys, n, n_slots, hash_kind);
          ++tables;
          // up to 8 threads, the entries dealt out round robin, every second thread from the back
          const uint32_t workers = 1 + below(8);
          for (uint64_t q = 0; q < n_slots; ++q) slots[q].store(kCollapseEmpty, std::memory_order_relaxed);
          std::atomic<uint32_t> failed{0};
          std::vector<std::thread> pool;
          for (uint32_t w = 0; w < workers; ++w) {
            pool.emplace_back([&, w]() {
              HostMem m{slots.get()};
              std::vector<uint32_t> mine;
              for (uint32_t i = w; i < n; i += workers) mine.push_back(i);
              if (w & 1) std::reverse(mine.begin(), mine.end());
              for (uint32_t i : mine)
                if (!collapse_insert(m, n_slots, hash_of(keys, i, hash_kind, n_slots), i, Same{keys, i})) failed.store(1, std::memory_order_relaxed);
            });
          }
          for (std::thread& t : pool) t.join();
          CHECK(failed.load() == 0);
          check_table(mem, keys, n, n_slots, hash_kind);
          ++threaded;
        }
      }
    }
  }
  printf("ok tables=%llu inserts=%llu threaded=%llu\n", (unsigned long long)tables, (unsigned long long)inserts, (unsigned long long)threaded);
  return 0;
}
