// clusters.hip -- connected components of the within-k graph of one set of sequences (sassy_hip_hamming_clusters,
// sassy_hip_edit_clusters; DESIGN.md 5.10 "Clusters").  The graph has an edge {i, j}, i != j, where the self-mode pair call
// of the same distance has a record (i, j, strand); the answer is per sequence the smallest index of its component.  No record
// is ever made: the pair units' walks visit every unordered pair once and hand each candidate to a union step
// (cluster_step.h) on one array of n indices.
//
// Launches:
//   cluster_init_kernel      parent[i] = i
//   pairs_cluster_kernel /   the link pass, next to the walk it uses (hamming_pairs.hip: pairs_link_components;
//   edit_cluster_kernel      edit_pairs.hip: edit_link_components), grid = strips x chunks of the pair call's plan
//   cluster_flatten_kernel   label[i] = the root of i's tree -- its component's minimum, whatever the link pass's schedule
// then the labels' copy back and one pass of the host over them for the sizes and the count.  There is no cell matrix, no
// rows pass, no scan, no fill.
#include <hip/hip_runtime.h>

#include <cstring>

#include "cluster_step.h"
#include "host_internal.h"

namespace sassy_hip {
namespace {

__global__ __launch_bounds__(256) void cluster_init_kernel(uint32_t* parent, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = (uint32_t)i;
}

// (the chase lowers what it passes: harmless beside other lanes' chases, cluster_step.h)
__global__ __launch_bounds__(256) void cluster_flatten_kernel(uint32_t* parent, uint64_t n, uint32_t* label) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  ClusterDeviceMem mem{parent};
  label[i] = cluster_find(mem, (uint32_t)i);
}

// out_size[i] = the entries that share label[i] (may be NULL); *n_clusters = the roots (may be NULL): O(n), no table beside
// the caller's -- a root's entry counts, then every entry reads its root's
void cluster_sizes(const uint32_t* label, size_t n, uint32_t* out_size, size_t* n_clusters) {
  if (n_clusters) {
    size_t roots = 0;
    for (size_t i = 0; i < n; ++i) roots += label[i] == i;
    *n_clusters = roots;
  }
  if (!out_size) return;
  memset(out_size, 0, n * sizeof(uint32_t));
  for (size_t i = 0; i < n; ++i) ++out_size[label[i]];
  for (size_t i = 0; i < n; ++i) out_size[i] = out_size[label[i]];  // (label[i] is a root: its entry is not written over)
}

// Both entry points behind their names: the refusals of the self-mode pair call of the same distance, then init, link,
// flatten, the copy back, the sizes.
int clusters_call(sassy_SearcherType* s, bool edit, const uint8_t* a, size_t n, size_t m, size_t k, uint32_t flags, uint32_t* out_label, uint32_t* out_size,
                  size_t* n_clusters, const char* who) {
  return pairs_guarded(who, [&]() -> int {
    if (int rc = edit ? edit_refusals(s, out_label != nullptr, a, n, m, nullptr, 0, 0, k, flags, who)
                      : pairs_refusals(s, out_label != nullptr, a, n, nullptr, 0, m, k, flags, who))
      return rc;
    const size_t lens[1] = {m};
    return hamming_call(s, lens, 1, k, [&](uint32_t kk) {  // (k >= m: every pair is an edge, one cluster)
      hipStream_t st = s->stream;
      s->stats.filtered = edit ? 11 : 10;
      if (int rc = s->d_pairs_out.reserve(n * 2 * sizeof(uint32_t))) return rc;
      uint32_t *d_parent = reinterpret_cast<uint32_t*>(s->d_pairs_out.p), *d_label = d_parent + n;
      const dim3 grid((uint32_t)((n + 255) / 256));
      hipLaunchKernelGGL(cluster_init_kernel, grid, dim3(256), 0, st, d_parent, (uint64_t)n);
      HIP_TRY(hipGetLastError());
      if (int rc = edit ? edit_link_components(s, a, n, (uint32_t)m, kk, d_parent) : pairs_link_components(s, a, n, (uint32_t)m, kk, d_parent)) return rc;
      hipLaunchKernelGGL(cluster_flatten_kernel, grid, dim3(256), 0, st, d_parent, (uint64_t)n, d_label);
      HIP_TRY(hipGetLastError());
      if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[2], st));
      HIP_TRY(hipMemcpyAsync(out_label, d_label, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      pairs_times(s, false);  // filter_ms the link pass, scan_ms link + flatten (scan_launches = 1: the one walk)
      cluster_sizes(out_label, n, out_size, n_clusters);
      return 0;
    });
  });
}

}  // namespace
}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_hamming_clusters(sassy_SearcherType* s, const uint8_t* a, size_t n, size_t m, size_t k, uint32_t flags, uint32_t* out_label, uint32_t* out_size,
                               size_t* n_clusters) {
  return clusters_call(s, false, a, n, m, k, flags, out_label, out_size, n_clusters, "hamming_clusters");
}

int sassy_hip_edit_clusters(sassy_SearcherType* s, const uint8_t* a, size_t n, size_t m, size_t k, uint32_t flags, uint32_t* out_label, uint32_t* out_size,
                            size_t* n_clusters) {
  return clusters_call(s, true, a, n, m, k, flags, out_label, out_size, n_clusters, "edit_clusters");
}

}  // extern "C"
