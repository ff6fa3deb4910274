// cluster_step_driver.cc -- drives sassy_amd/csrc/cluster_step.h (the union step of sassy_hip_hamming_clusters /
// sassy_hip_edit_clusters, free of HIP) on the host, its memory policy instantiated with std::atomic.  Random edge lists --
// paths, stars, cliques, forests and mixtures of them under a random renaming of the indices -- are linked edge by edge and
// checked against a sequential union-find: parent[x] <= x after every link, no value ever rises, the root of every tree is
// the minimum of its component at the end.  Then the same edges are linked from up to 8 threads in shuffled order, half of
// them through cluster_join with a register as the kernels hold it, and must give the identical label array.
// Built by tests/test_clusters_cpu.py with -fsanitize=address,undefined and again with -fsanitize=thread.
//   cluster_step_driver <seed>   prints "ok graphs=<n> links=<n> threaded=<n>", exit status 0;
//                                a failed check: its line on stderr, 1
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <thread>
#include <utility>
#include <vector>

#include "../../sassy_amd/csrc/cluster_step.h"

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

// the policy of cluster_step.h over std::atomic, relaxed
struct HostMem {
  std::atomic<uint32_t>* parent;
  uint32_t load(uint32_t x) const { return parent[x].load(std::memory_order_relaxed); }
  bool cas(uint32_t x, uint32_t expect, uint32_t desired) const {
    return parent[x].compare_exchange_strong(expect, desired, std::memory_order_relaxed, std::memory_order_relaxed);
  }
};

typedef std::pair<uint32_t, uint32_t> Edge;

// the reference: a sequential union-find, label = component minimum
static std::vector<uint32_t> reference_labels(uint32_t n, const std::vector<Edge>& edges) {
  std::vector<uint32_t> p(n);
  for (uint32_t x = 0; x < n; ++x) p[x] = x;
  auto find = [&](uint32_t x) {
    while (p[x] != x) x = p[x] = p[p[x]];
    return x;
  };
  for (const Edge& e : edges) {
    const uint32_t a = find(e.first), b = find(e.second);
    if (a != b) p[std::max(a, b)] = std::min(a, b);
  }
  std::vector<uint32_t> label(n);
  for (uint32_t x = 0; x < n; ++x) label[x] = find(x);
  for (uint32_t x = 0; x < n; ++x) CHECK(label[x] <= x && label[label[x]] == label[x]);
  return label;
}

// kind 0: one path; 1: stars; 2: cliques; 3: a forest of random trees; 4: a mixture with random extra edges
static std::vector<Edge> make_graph(uint32_t kind, uint32_t n) {
  std::vector<Edge> e;
  if (n < 2) return e;
  if (kind == 0) {
    for (uint32_t x = 0; x + 1 < n; ++x) e.push_back(Edge(x, x + 1));
  } else if (kind == 1) {
    const uint32_t hubs = 1 + below(4);
    for (uint32_t x = hubs; x < n; ++x)
      if (below(8)) e.push_back(Edge(x % hubs, x));
  } else if (kind == 2) {
    const uint32_t size = 2 + below(24);
    for (uint32_t c0 = 0; c0 < n; c0 += size)
      for (uint32_t x = c0; x < std::min(n, c0 + size); ++x)
        for (uint32_t y = x + 1; y < std::min(n, c0 + size); ++y) e.push_back(Edge(x, y));
  } else if (kind == 3) {
    for (uint32_t x = 1; x < n; ++x)
      if (below(10)) e.push_back(Edge(below(x), x));  // (a tree edge to an earlier node; one in ten starts a new tree)
  } else {
    for (uint32_t x = 1; x < n; ++x)
      if (below(3) == 0) e.push_back(Edge(below(x), x));
    for (uint32_t q = 0; q < n / 4; ++q) {
      const uint32_t x = below(n), y = below(n);
      if (x != y) e.push_back(Edge(x, y));
    }
  }
  // a random renaming of the indices and a random order and orientation of the edges
  std::vector<uint32_t> name(n);
  for (uint32_t x = 0; x < n; ++x) name[x] = x;
  shuffle(name);
  for (Edge& d : e) {
    d = Edge(name[d.first], name[d.second]);
    if (below(2)) std::swap(d.first, d.second);
  }
  shuffle(e);
  return e;
}

static void reset(std::atomic<uint32_t>* parent, uint32_t n) {
  for (uint32_t x = 0; x < n; ++x) parent[x].store(x, std::memory_order_relaxed);
}
static void check_labels(HostMem& mem, uint32_t n, const std::vector<uint32_t>& want) {
  for (uint32_t x = 0; x < n; ++x) CHECK(mem.load(x) <= x);
  for (uint32_t x = 0; x < n; ++x) CHECK(cluster_find(mem, x) == want[x]);
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  static const uint32_t kSizes[] = {1, 2, 3, 64, 65, 257, 1000, 4000};
  uint64_t graphs = 0, links = 0, threaded = 0;
  for (uint32_t kind = 0; kind < 5; ++kind) {
    for (uint32_t n : kSizes) {
      const std::vector<Edge> edges = make_graph(kind, n);
      const std::vector<uint32_t> want = reference_labels(n, edges);
      std::unique_ptr<std::atomic<uint32_t>[]> parent(new std::atomic<uint32_t>[n]);
      HostMem mem{parent.get()};
      // one thread, edge by edge: the invariants after every link (all of them for small n, the two trees' nodes else)
      reset(parent.get(), n);
      std::vector<uint32_t> before(n);
      for (uint32_t x = 0; x < n; ++x) before[x] = x;
      for (const Edge& d : edges) {
        const uint32_t r = cluster_link(mem, d.first, d.second);
        ++links;
        CHECK(r <= d.first && r <= d.second);
        CHECK(cluster_find(mem, d.first) == cluster_find(mem, d.second));
        if (n <= 300) {
          for (uint32_t x = 0; x < n; ++x) {
            const uint32_t p = mem.load(x);
            CHECK(p <= x && p <= before[x]);  // (no value ever rises)
            before[x] = p;
          }
        } else {
          CHECK(mem.load(d.first) <= d.first && mem.load(d.second) <= d.second);
        }
      }
      check_labels(mem, n, want);
      ++graphs;
      // up to 8 threads, the edges dealt out in another order; every second thread as a kernel's lane does it, one entry with
      // its register through cluster_join
      const uint32_t workers = 1 + below(8);
      std::vector<Edge> dealt = edges;
      shuffle(dealt);
      reset(parent.get(), n);
      std::vector<std::thread> pool;
      for (uint32_t w = 0; w < workers; ++w) {
        pool.emplace_back([&, w]() {
          HostMem m{parent.get()};
          uint32_t owner = 0xFFFFFFFFu, root = 0;
          for (size_t q = w; q < dealt.size(); q += workers) {
            const Edge d = dealt[q];
            if (w & 1) {
              if (owner != d.first) {
                owner = d.first;
                root = d.first;
              }
              cluster_join(m, d.first, d.second, root);
            } else {
              (void)cluster_link(m, d.first, d.second);
              cluster_lower(m, d.second, cluster_find(m, d.first));
            }
          }
        });
      }
      for (std::thread& t : pool) t.join();
      check_labels(mem, n, want);
      ++threaded;
    }
  }
  printf("ok graphs=%llu links=%llu threaded=%llu\n", (unsigned long long)graphs, (unsigned long long)links, (unsigned long long)threaded);
  return 0;
}
