// umi_step_driver.cc -- drives sassy_amd/csrc/umi_step.h (the directional rule of sassy_hip_umi_groups, free of HIP) on the
// host, its memory policy instantiated with std::atomic.  Counted sequences with neighbour pairs -- paths (all of count 1,
// falling counts, rising counts), stars (an abundant hub, a rare hub), and random pairs with random counts, all under a random
// renaming -- are relaxed pass by pass over the records until a pass lowers nothing, as the host loop of umi_groups.hip does,
// and the fixpoint is checked against the SEQUENTIAL procedure: sort by (count descending, index ascending), open a group at
// the first sequence without one, take what a breadth-first search along the count-rule edges reaches.  The number of passes
// stays within n + 1.  Then the same passes with the records dealt out to up to 8 threads (a join between passes, as a
// kernel boundary is) must reach the identical labels.
// Built by tests/test_umi_groups_cpu.py with -fsanitize=address,undefined and again with -fsanitize=thread.
//   umi_step_driver <seed>   prints "ok graphs=<n> relaxes=<n> threaded=<n> longest=<passes>", exit status 0;
//                            a failed check: its line on stderr, 1
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <memory>
#include <thread>
#include <utility>
#include <vector>

#include "../../sassy_amd/csrc/umi_step.h"

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
template <typename T>
static void shuffle(std::vector<T>& v) {
  for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[below((uint32_t)i)]);
}

// the policy of umi_step.h over std::atomic, relaxed
struct HostMem {
  std::atomic<uint64_t>* label;
  uint64_t load(uint32_t x) const { return label[x].load(std::memory_order_relaxed); }
  uint64_t fetch_min(uint32_t x, uint64_t value) const {
    uint64_t seen = label[x].load(std::memory_order_relaxed);
    while (value < seen && !label[x].compare_exchange_weak(seen, value, std::memory_order_relaxed, std::memory_order_relaxed)) {
    }
    return seen;
  }
};

typedef std::pair<uint32_t, uint32_t> Pair;
struct Graph {
  std::vector<uint32_t> count;
  std::vector<Pair> pairs;  // neighbours, u != v
};

// kind 0: a path of count-1 sequences; 1: a path of falling counts (edges one way); 2: a path of slowly rising counts;
// 3: stars with abundant hubs; 4: stars with rare hubs; 5, 6: random pairs, random counts (6: heavy-tailed)
static Graph make_graph(uint32_t kind, uint32_t n) {
  Graph g;
  g.count.assign(n, 1);
  if (kind <= 2) {
    for (uint32_t x = 0; x + 1 < n; ++x) g.pairs.push_back(Pair(x, x + 1));
    if (kind == 1)
      for (uint32_t x = 0; x < n; ++x) g.count[x] = 3 * (n - x);
    if (kind == 2)
      for (uint32_t x = 0; x < n; ++x) g.count[x] = 1 + x / 3;
  } else if (kind <= 4) {
    const uint32_t hubs = 1 + below(4);
    for (uint32_t x = hubs; x < n; ++x)
      if (below(8)) g.pairs.push_back(Pair(x % hubs, x));
    for (uint32_t x = 0; x < n; ++x) g.count[x] = (x < hubs) == (kind == 3) ? 20 + below(5) : 1 + below(3);
  } else {
    for (uint32_t x = 0; x < n; ++x) g.count[x] = kind == 5 ? 1 + below(8) : below(10) ? 1 + below(2) : 1 + below(200);
    for (uint32_t q = 0; q < n + n / 2; ++q) {
      const uint32_t x = below(n), y = below(n);
      if (x != y) g.pairs.push_back(Pair(x, y));
    }
  }
  // a random renaming of the indices, a random order and orientation of the pairs
  std::vector<uint32_t> name(n);
  for (uint32_t x = 0; x < n; ++x) name[x] = x;
  shuffle(name);
  std::vector<uint32_t> count(n);
  for (uint32_t x = 0; x < n; ++x) count[name[x]] = g.count[x];
  g.count = count;
  for (Pair& p : g.pairs) {
    p = Pair(name[p.first], name[p.second]);
    if (below(2)) std::swap(p.first, p.second);
  }
  shuffle(g.pairs);
  return g;
}

// the reference: UMI-tools' sequential procedure
static std::vector<uint32_t> reference_openers(const Graph& g) {
  const uint32_t n = (uint32_t)g.count.size();
  std::vector<std::vector<uint32_t>> out(n);
  for (const Pair& p : g.pairs) {
    if ((uint64_t)g.count[p.first] >= 2 * (uint64_t)g.count[p.second] - 1) out[p.first].push_back(p.second);
    if ((uint64_t)g.count[p.second] >= 2 * (uint64_t)g.count[p.first] - 1) out[p.second].push_back(p.first);
  }
  std::vector<uint32_t> order(n);
  for (uint32_t x = 0; x < n; ++x) order[x] = x;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return g.count[x] != g.count[y] ? g.count[x] > g.count[y] : x < y; });
  const uint32_t none = 0xFFFFFFFFu;
  std::vector<uint32_t> opener(n, none);
  for (uint32_t u : order) {
    if (opener[u] != none) continue;
    opener[u] = u;
    std::deque<uint32_t> queue(1, u);
    while (!queue.empty()) {
      const uint32_t x = queue.front();
      queue.pop_front();
      for (uint32_t y : out[x])
        if (opener[y] == none) {
          opener[y] = u;
          queue.push_back(y);
        }
    }
  }
  return opener;
}

static void reset(std::atomic<uint64_t>* label, const Graph& g) {
  for (uint32_t x = 0; x < g.count.size(); ++x) label[x].store(umi_key(g.count[x], x), std::memory_order_relaxed);
}
static void check_labels(HostMem& mem, const Graph& g, const std::vector<uint32_t>& want) {
  for (uint32_t x = 0; x < g.count.size(); ++x) CHECK(umi_key_index(mem.load(x)) == want[x] && mem.load(x) == umi_key(g.count[want[x]], want[x]));
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  static const uint32_t kSizes[] = {1, 2, 3, 64, 65, 129, 257, 1000, 4000};
  uint64_t graphs = 0, relaxes = 0, threaded = 0, longest = 0;
  CHECK(umi_absorbs(1, 1) && umi_absorbs(7, 4) && !umi_absorbs(6, 4) && umi_absorbs(3, 2) && !umi_absorbs(2, 2) && umi_absorbs(0x7FFFFFFFu, 0x40000000u));
  CHECK(umi_key(5, 9) < umi_key(4, 0) && umi_key(5, 3) < umi_key(5, 4) && umi_key_index(umi_key(5, 9)) == 9);
  for (uint32_t kind = 0; kind < 7; ++kind) {
    for (uint32_t n : kSizes) {
      const Graph g = make_graph(kind, n);
      const std::vector<uint32_t> want = reference_openers(g);
      std::unique_ptr<std::atomic<uint64_t>[]> label(new std::atomic<uint64_t>[n]);
      HostMem mem{label.get()};
      // one thread: passes over the records until one lowers nothing; no label ever rises
      reset(label.get(), g);
      std::vector<uint64_t> before(n);
      for (uint32_t x = 0; x < n; ++x) before[x] = mem.load(x);
      uint64_t passes = 0;
      for (bool fell = true; fell;) {
        CHECK(passes <= n);  // (at most n + 1 passes)
        fell = false;
        for (const Pair& p : g.pairs) {
          fell |= umi_relax(mem, p.first, p.second, g.count[p.first], g.count[p.second]);
          ++relaxes;
        }
        ++passes;
        for (uint32_t x = 0; x < n; ++x) {
          CHECK(mem.load(x) <= before[x]);
          before[x] = mem.load(x);
        }
      }
      longest = std::max(longest, passes);
      check_labels(mem, g, want);
      ++graphs;
      // up to 8 threads per pass, the records dealt out round robin in another order
      const uint32_t workers = 1 + below(8);
      std::vector<Pair> dealt = g.pairs;
      shuffle(dealt);
      reset(label.get(), g);
      passes = 0;
      for (std::atomic<uint32_t> fell{1}; fell.load();) {
        CHECK(passes <= n);
        fell.store(0);
        std::vector<std::thread> pool;
        for (uint32_t w = 0; w < workers; ++w) {
          pool.emplace_back([&, w]() {
            HostMem m{label.get()};
            for (size_t q = w; q < dealt.size(); q += workers)
              if (umi_relax(m, dealt[q].first, dealt[q].second, g.count[dealt[q].first], g.count[dealt[q].second])) fell.store(1, std::memory_order_relaxed);
          });
        }
        for (std::thread& t : pool) t.join();
        ++passes;
      }
      check_labels(mem, g, want);
      ++threaded;
    }
  }
  printf("ok graphs=%llu relaxes=%llu threaded=%llu longest=%llu\n", (unsigned long long)graphs, (unsigned long long)relaxes, (unsigned long long)threaded,
         (unsigned long long)longest);
  return 0;
}
