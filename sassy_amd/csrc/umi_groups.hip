// umi_groups.hip -- UMI grouping of one list of equal-length sequences (sassy_hip_umi_groups; DESIGN.md 5.10 "UMI groups"):
// identical reads are counted and collapsed on the device, the pair walk of hamming_pairs.hip runs over the DISTINCT
// sequences only, and the groups are their connected components (CLUSTER) or what UMI-tools' directional rule makes of
// them (DIRECTIONAL: an abundant sequence absorbs a rare neighbour, two abundant ones never join).  The table's rules are
// collapse_step.h's, the directional rule is umi_step.h's, the component forest cluster_step.h's.
//
// Launches, one thread per read unless said otherwise; no record and no label goes to the host between them:
//   umi_insert_kernel    every read into the duplicate table, keyed by its plane words (collapse_step.h)
//   umi_lookup_kernel    rep[i] = the table's final value for i's class, count[rep[i]] += 1, flag[i] = (rep[i] == i)
//   pairs_scan_*_kernel  the exclusive scan of the flags (hamming_pairs.hip: pairs_scan_u64): dense[i], the number of distinct
//                        sequences before i -- the distinct sequences' numbering in ascending first index; its total is n_u
//   umi_gather_kernel    per distinct sequence u = dense[i]: first[u] = i, cnt[u] = count[i], its planes (and both target
//                        records of an rc searcher) into arrays of n_u entries
//   CLUSTER:      umi_init_kernel, pairs_cluster_kernel over the n_u arrays (pairs_resident_link); the group kernel flattens
//   DIRECTIONAL:  survey, rows, scan, fill over the n_u arrays (pairs_resident_records; the records stay on the device),
//                 umi_init_kernel, then umi_relax_kernel -- one thread per record -- until a launch lowers nothing
//   umi_group_kernel     per distinct sequence: its group g (dense), size[g] += cnt[u] -- one atomic per DISTINCT sequence
//   umi_expand_kernel    per read: label = first[g of dense[rep[i]]], size = size[g], rep, count = count[rep[i]]
// then the four columns' copy back and one pass of the host over the labels for *n_groups.  The sizes are made on the
// device (umi_group_kernel's adds, read back by umi_expand_kernel); the host's cluster_sizes pass is not used.
#include <hip/hip_runtime.h>

#include <cstring>

#include "cluster_step.h"
#include "collapse_step.h"
#include "host_internal.h"
#include "pairs_step.h"
#include "umi_step.h"

namespace sassy_hip {
namespace {

// collapse_step.h's memory policy on the device: relaxed, agent scope, vector memory operations
struct CollapseDeviceMem {
  uint32_t* slots;
  __device__ __forceinline__ uint32_t load(uint64_t x) const { return __hip_atomic_load(slots + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ uint32_t cas(uint64_t x, uint32_t expect, uint32_t desired) const {
    (void)__hip_atomic_compare_exchange_strong(slots + x, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;  // (what the slot held: the builtin leaves it here when the swap was refused)
  }
  __device__ __forceinline__ uint32_t fetch_min(uint64_t x, uint32_t value) const {
    return __hip_atomic_fetch_min(slots + x, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
// umi_step.h's
struct UmiDeviceMem {
  unsigned long long* label;
  __device__ __forceinline__ uint64_t load(uint32_t x) const { return __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ uint64_t fetch_min(uint32_t x, uint64_t value) const {
    return __hip_atomic_fetch_min(label + x, (unsigned long long)value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// Entry i's key against entry v's: PW plane words each (read-only for the whole call)
template <int PW>
struct SameKey {
  const uint32_t* planes;
  const uint32_t (&mine)[PW];
  __device__ __forceinline__ bool operator()(uint32_t v) const {
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < PW; ++q) diff |= planes[(size_t)v * PW + q] ^ mine[q];
    return diff == 0;
  }
};

struct CollapseArgs {
  const uint32_t* planes;  // [n][PW]
  uint64_t n, n_slots;
  uint32_t* slots;
  uint32_t *rep, *count;   // [n]
  unsigned long long* flag;  // [n]: rep[i] == i
  uint32_t* error;         // raised where a probe sequence ran out (an internal error: n_slots >= n rules it out)
};

template <int PW>
__global__ __launch_bounds__(256) void umi_insert_kernel(CollapseArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  uint32_t mine[PW];
#pragma unroll
  for (int q = 0; q < PW; ++q) mine[q] = A.planes[(size_t)i * PW + q];
  CollapseDeviceMem mem{A.slots};
  if (!collapse_insert(mem, A.n_slots, collapse_hash(mine, PW), (uint32_t)i, SameKey<PW>{A.planes, mine}))
    __hip_atomic_store(A.error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int PW>
__global__ __launch_bounds__(256) void umi_lookup_kernel(CollapseArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  uint32_t mine[PW];
#pragma unroll
  for (int q = 0; q < PW; ++q) mine[q] = A.planes[(size_t)i * PW + q];
  CollapseDeviceMem mem{A.slots};
  uint32_t r = collapse_lookup(mem, A.n_slots, collapse_hash(mine, PW), (uint32_t)i, SameKey<PW>{A.planes, mine});
  if (r == kCollapseEmpty) {  // (never: every read was inserted)
    __hip_atomic_store(A.error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    r = (uint32_t)i;
  }
  A.rep[i] = r;
  A.flag[i] = r == (uint32_t)i ? 1ull : 0ull;
  (void)__hip_atomic_fetch_add(A.count + r, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct GatherArgs {
  const uint32_t *planes, *targets;  // [n][PW], [n][S][PW]
  const uint32_t *rep, *count;
  const unsigned long long* dense;
  uint64_t n;
  uint32_t PW, SPW;                  // words per entry, per entry's target records (0: no planes are gathered)
  uint32_t *first, *cnt;             // [n_u]
  uint32_t *u_planes, *u_targets;    // [n_u][PW], [n_u][S][PW] (u_targets == NULL: one strand, the planes serve)
};
__global__ __launch_bounds__(256) void umi_gather_kernel(GatherArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n || A.rep[i] != (uint32_t)i) return;
  const uint64_t u = A.dense[i];
  A.first[u] = (uint32_t)i;
  A.cnt[u] = A.count[i];
  if (A.u_planes)
    for (uint32_t q = 0; q < A.PW; ++q) A.u_planes[u * A.PW + q] = A.planes[i * A.PW + q];
  if (A.u_targets)
    for (uint32_t q = 0; q < A.SPW; ++q) A.u_targets[u * A.SPW + q] = A.targets[i * A.SPW + q];
}

// parent[u] = u (CLUSTER), label64[u] = key[u] (DIRECTIONAL), size[u] = 0
__global__ __launch_bounds__(256) void umi_init_kernel(uint64_t n_u, const uint32_t* cnt, uint32_t* parent, unsigned long long* label64, uint32_t* size) {
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= n_u) return;
  if (parent) parent[u] = (uint32_t)u;
  if (label64) label64[u] = umi_key(cnt[u], (uint32_t)u);
  size[u] = 0;
}

// one neighbour record per thread (the pair call's records of the distinct sequences; (u, u, 1) is no edge)
__global__ __launch_bounds__(256) void umi_relax_kernel(const sassy_hip_HammingPair* rec, uint64_t n_rec, const uint32_t* cnt, unsigned long long* label64,
                                                        uint32_t* changed) {
  const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n_rec) return;
  const uint32_t u = rec[q].a_idx, v = rec[q].b_idx;
  if (u == v) return;
  UmiDeviceMem mem{label64};
  if (umi_relax(mem, u, v, cnt[u], cnt[v])) __hip_atomic_store(changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// group[u]: the dense number of u's group's label; size[group[u]] += cnt[u].  parent: CLUSTER (the chase lowers what it
// passes: harmless beside other lanes' chases, cluster_step.h); label64: DIRECTIONAL; neither: UNIQUE
__global__ __launch_bounds__(256) void umi_group_kernel(uint64_t n_u, const uint32_t* cnt, uint32_t* parent, const unsigned long long* label64, uint32_t* group,
                                                        uint32_t* size) {
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= n_u) return;
  uint32_t g = (uint32_t)u;
  if (parent) {
    ClusterDeviceMem mem{parent};
    g = cluster_find(mem, (uint32_t)u);
  } else if (label64) {
    g = umi_key_index(label64[u]);
  }
  group[u] = g;
  (void)__hip_atomic_fetch_add(size + g, cnt[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct ExpandArgs {
  uint64_t n;
  const uint32_t *rep, *count;
  const unsigned long long* dense;
  const uint32_t *first, *group, *size;  // [n_u]
  uint32_t *out_label, *out_size, *out_count;
};
__global__ __launch_bounds__(256) void umi_expand_kernel(ExpandArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t r = A.rep[i];
  const uint32_t g = A.group[A.dense[r]];
  A.out_label[i] = A.first[g];
  A.out_size[i] = A.size[g];
  A.out_count[i] = A.count[r];
}

template <int PW>
hipError_t launch_collapse(const CollapseArgs& A, hipStream_t st) {
  const dim3 grid((uint32_t)((A.n + 255) / 256));
  hipLaunchKernelGGL(umi_insert_kernel<PW>, grid, dim3(256), 0, st, A);
  hipLaunchKernelGGL(umi_lookup_kernel<PW>, grid, dim3(256), 0, st, A);
  return hipGetLastError();
}
hipError_t launch_collapse_words(uint32_t PW, const CollapseArgs& A, hipStream_t st) {
  switch (PW) {  // P in {2, 4, 8} x W in {1, 2, 4}
    case 2: return launch_collapse<2>(A, st);
    case 4: return launch_collapse<4>(A, st);
    case 8: return launch_collapse<8>(A, st);
    case 16: return launch_collapse<16>(A, st);
    default: return launch_collapse<32>(A, st);
  }
}

size_t round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
// carves arrays out of one device buffer, 16-byte aligned
struct Carver {
  uint8_t* base = nullptr;
  size_t used = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += round16(count * sizeof(T));
    return p;
  }
};

// what is sized by the reads
struct ReadArrays {
  uint32_t *slots, *rep, *count, *out_label, *out_size, *out_count, *flags;
  unsigned long long *flag, *dense, *block_sum;
  void carve(Carver& c, size_t n, size_t n_slots) {
    slots = c.take<uint32_t>(n_slots);
    rep = c.take<uint32_t>(n);
    count = c.take<uint32_t>(n);
    out_label = c.take<uint32_t>(n);
    out_size = c.take<uint32_t>(n);
    out_count = c.take<uint32_t>(n);
    flag = c.take<unsigned long long>(n);
    dense = c.take<unsigned long long>(n);
    block_sum = c.take<unsigned long long>(pairs_scan_blocks(n) + 1);
    flags = c.take<uint32_t>(4);  // [0] the collapse's error flag, [1] the relaxation's "something fell"
  }
};
// what is sized by the distinct sequences
struct DistinctArrays {
  uint32_t *first, *cnt, *group, *size, *parent, *planes, *targets;
  unsigned long long* label64;
  void carve(Carver& c, size_t n_u, size_t PW, size_t S, uint32_t method) {
    first = c.take<uint32_t>(n_u);
    cnt = c.take<uint32_t>(n_u);
    group = c.take<uint32_t>(n_u);
    size = c.take<uint32_t>(n_u);
    parent = method == SASSY_HIP_UMI_CLUSTER ? c.take<uint32_t>(n_u) : nullptr;
    label64 = method == SASSY_HIP_UMI_DIRECTIONAL ? c.take<unsigned long long>(n_u) : nullptr;
    planes = method != SASSY_HIP_UMI_UNIQUE ? c.take<uint32_t>(n_u * PW) : nullptr;
    targets = method != SASSY_HIP_UMI_UNIQUE && S == 2 ? c.take<uint32_t>(n_u * S * PW) : nullptr;
  }
};

}  // namespace

// The call behind its refusals and behind the list's upload (host_internal.h; dedup_reads.hip calls it over planes that a kernel
// made): d_planes [n][P W], d_targets [S n][P W] lie on the device (an rc searcher reads d_targets; one strand: the planes
// serve).  out_label == NULL: no column goes to the host and *n_groups is left alone.  dev, where given: where the four columns
// lie on the device until the searcher's next grouping call.  Timing level 2: ev_line[0] -> [1] the collapse (the table's
// clearing, insert, lookup, scan, gather), [1] -> [2] the walk passes over the distinct sequences, [2] -> [3] the relaxation
// (CLUSTER: the flatten) with the group and expand kernels.
int umi_groups_resident(sassy_SearcherType* s, const uint32_t* d_planes, const uint32_t* d_targets, size_t n, uint32_t m, uint32_t k, uint32_t method,
                        uint32_t* out_label, uint32_t* out_size, uint32_t* out_rep, uint32_t* out_count, size_t* n_unique, size_t* n_groups,
                        UmiColumns* dev) {
  hipStream_t st = s->stream;
  const char* who = "umi_groups";
  s->stats.filtered = 12;
  const uint32_t S = s->rc ? 2u : 1u, PW = pairs_planes(s->profile) * pairs_words(m);

  // ---- the collapse ----
  const uint64_t n_slots = collapse_slots_for(n, s->sw.collapse_slots);
  ReadArrays R;
  {
    Carver sizing;
    R.carve(sizing, n, n_slots);
    if (int rc = s->d_umi_reads.reserve(sizing.used)) return rc;
    Carver c{s->d_umi_reads.p};
    R.carve(c, n, n_slots);
  }
  const dim3 read_grid((uint32_t)((n + 255) / 256));
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[0], st));
  HIP_TRY(hipMemsetAsync(R.slots, 0xFF, n_slots * sizeof(uint32_t), st));  // (kCollapseEmpty)
  HIP_TRY(hipMemsetAsync(R.count, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(R.flags, 0, 4 * sizeof(uint32_t), st));
  CollapseArgs CA{d_planes, n, n_slots, R.slots, R.rep, R.count, R.flag, R.flags};
  HIP_TRY(launch_collapse_words(PW, CA, st));
  if (int rc = pairs_scan_u64(s, R.flag, n, R.block_sum, R.dense)) return rc;
  unsigned long long n_u = 0;
  uint32_t collapse_error = 0;
  HIP_TRY(hipMemcpyAsync(&n_u, R.block_sum + pairs_scan_blocks(n), 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&collapse_error, R.flags, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (collapse_error || n_u == 0 || n_u > n) return fail(SASSY_HIP_EINVAL, "umi_groups: the duplicate table lost an entry (internal error)");
  DistinctArrays D;
  {
    Carver sizing;
    D.carve(sizing, n_u, PW, S, method);
    if (int rc = s->d_umi_distinct.reserve(sizing.used)) return rc;
    Carver c{s->d_umi_distinct.p};
    D.carve(c, n_u, PW, S, method);
  }
  GatherArgs GA{d_planes, d_targets, R.rep, R.count, R.dense, n, PW, S * PW, D.first, D.cnt, D.planes, D.targets};
  hipLaunchKernelGGL(umi_gather_kernel, read_grid, dim3(256), 0, st, GA);
  const dim3 distinct_grid((uint32_t)((n_u + 255) / 256));
  hipLaunchKernelGGL(umi_init_kernel, distinct_grid, dim3(256), 0, st, (uint64_t)n_u, D.cnt, D.parent, D.label64, D.size);
  HIP_TRY(hipGetLastError());
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[1], st));

  // ---- the walk over the distinct sequences (one strand: the entries' planes are the target records) ----
  const uint32_t* u_targets = S == 2 ? D.targets : D.planes;
  unsigned long long n_rec = 0;
  if (method == SASSY_HIP_UMI_CLUSTER) {
    if (int rc = pairs_resident_link(s, D.planes, u_targets, n_u, m, k, D.parent)) return rc;
  } else if (method == SASSY_HIP_UMI_DIRECTIONAL) {
    if (int rc = pairs_resident_records(s, D.planes, u_targets, n_u, m, k, who, &n_rec)) return rc;
  } else {
    s->stats.scan_launches = 0;
  }
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[2], st));  // (again, behind the rows pass's own record of it)

  // ---- DIRECTIONAL: relax until a launch lowers nothing ----
  uint64_t rounds = 0;
  if (method == SASSY_HIP_UMI_DIRECTIONAL && n_rec) {
    const sassy_hip_HammingPair* rec = reinterpret_cast<const sassy_hip_HammingPair*>(s->d_pairs_out.p);
    const dim3 rec_grid((uint32_t)((n_rec + 255) / 256));
    for (;;) {
      // a launch hands every label at least one edge further (umi_step.h), so launch n_u at the latest lowers nothing:
      // beyond n_u + 1 something is wrong, and the loop does not spin
      if (rounds > n_u) return fail(SASSY_HIP_EINVAL, "umi_groups: the relaxation did not settle in " + std::to_string(n_u + 1) + " launches (internal error)");
      uint32_t changed = 0;
      HIP_TRY(hipMemsetAsync(R.flags + 1, 0, sizeof(uint32_t), st));
      hipLaunchKernelGGL(umi_relax_kernel, rec_grid, dim3(256), 0, st, rec, (uint64_t)n_rec, D.cnt, D.label64, R.flags + 1);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&changed, R.flags + 1, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      ++rounds;
      if (!changed) break;
    }
  }

  // ---- groups, sizes, the way back to the reads ----
  hipLaunchKernelGGL(umi_group_kernel, distinct_grid, dim3(256), 0, st, (uint64_t)n_u, D.cnt, D.parent, D.label64, D.group, D.size);
  ExpandArgs EA{n, R.rep, R.count, R.dense, D.first, D.group, D.size, R.out_label, R.out_size, R.out_count};
  hipLaunchKernelGGL(umi_expand_kernel, read_grid, dim3(256), 0, st, EA);
  HIP_TRY(hipGetLastError());
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[3], st));
  if (out_label) HIP_TRY(hipMemcpyAsync(out_label, R.out_label, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (out_size) HIP_TRY(hipMemcpyAsync(out_size, R.out_size, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (out_rep) HIP_TRY(hipMemcpyAsync(out_rep, R.rep, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (out_count) HIP_TRY(hipMemcpyAsync(out_count, R.out_count, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (s->timing >= 2) {
    float collapse = 0, walk = 0, last = 0;
    (void)hipEventElapsedTime(&collapse, s->ev_line[0], s->ev_line[1]);
    (void)hipEventElapsedTime(&walk, s->ev_line[1], s->ev_line[2]);
    (void)hipEventElapsedTime(&last, s->ev_line[2], s->ev_line[3]);
    s->stats.filter_ms = walk;
    s->stats.trace_ms = last;
    s->stats.scan_ms = (double)collapse + walk + last;  // (the collapse: scan_ms - filter_ms - trace_ms)
  }
  s->stats.candidates = n_rec;
  s->stats.hit_blocks = n_u;
  s->stats.blocks = rounds;
  s->stats.text_bytes = (uint64_t)n * m;
  if (n_unique) *n_unique = (size_t)n_u;
  if (n_groups && out_label) {
    size_t roots = 0;
    for (size_t i = 0; i < n; ++i) roots += out_label[i] == i;
    *n_groups = roots;
  }
  if (dev) *dev = UmiColumns{R.out_label, R.out_size, R.rep, R.out_count};
  return 0;
}

namespace {
// the list's upload, then the part above
int umi_run(sassy_SearcherType* s, const uint8_t* a, size_t n, uint32_t m, uint32_t k, uint32_t method, uint32_t* out_label, uint32_t* out_size,
            uint32_t* out_rep, uint32_t* out_count, size_t* n_unique, size_t* n_groups) {
  const uint32_t *d_planes = nullptr, *d_targets = nullptr;
  if (int rc = pairs_upload_self(s, a, n, m, &d_planes, &d_targets)) return rc;
  return umi_groups_resident(s, d_planes, d_targets, n, m, k, method, out_label, out_size, out_rep, out_count, n_unique, n_groups, nullptr);
}

}  // namespace
}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_umi_groups(sassy_SearcherType* s, const uint8_t* a, size_t n, size_t m, size_t k, uint32_t method, uint32_t flags, uint32_t* out_label,
                         uint32_t* out_size, uint32_t* out_rep, uint32_t* out_count, size_t* n_unique, size_t* n_groups) {
  const char* who = "umi_groups";
  return pairs_guarded(who, [&]() -> int {
    if (int rc = pairs_refusals(s, out_label != nullptr, a, n, nullptr, 0, m, k, flags, who)) return rc;
    if (method > SASSY_HIP_UMI_DIRECTIONAL)
      return fail(SASSY_HIP_EINVAL, "umi_groups: unknown method " + std::to_string(method) + " (0 unique, 1 cluster, 2 directional)");
    const size_t lens[1] = {m};
    return hamming_call(s, lens, 1, k, [&](uint32_t kk) {  // (k >= m: every two distinct sequences are neighbours)
      return umi_run(s, a, n, (uint32_t)m, kk, method, out_label, out_size, out_rep, out_count, n_unique, n_groups);
    });
  });
}

}  // extern "C"
