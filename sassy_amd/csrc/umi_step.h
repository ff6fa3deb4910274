// umi_step.h -- the directional rule of the UMI grouping call (umi_groups.hip: sassy_hip_umi_groups; DESIGN.md 5.10 "UMI
// groups"), free of HIP and of the environment: plain C++17 that the relax kernel and the host test driver
// (tests/c/umi_step_driver.cc) compile alike.
//
// Distinct sequences 0 .. n_u - 1 (numbered in ascending first index), each with a count c >= 1, and neighbour pairs {u, v}.
// There is an edge u -> v where they are neighbours and c_u >= 2 c_v - 1 (umi_absorbs).  The order of the sequences is
// (count descending, index ascending): key[u] = (0xFFFFFFFF - c_u) << 32 | u, smaller is earlier.  The sequential procedure --
// go through the sequences in that order, one that is in no group yet opens a group and takes everything reachable from it
// that is in no group yet -- labels v with the FIRST u in the order from which v is reachable (v itself included): such a u
// cannot have been taken by an earlier opener, which would reach v too.  So
//   label[v] = min { key[u] : v is reachable from u },
// and that is what the relaxation computes.  One array label64[0 .. n_u) that starts as label64[u] = key[u], behind a memory
// policy M of two relaxed operations:
//   uint64_t M::load(uint32_t x)                       the value of label64[x]
//   uint64_t M::fetch_min(uint32_t x, uint64_t value)   label64[x] = min(label64[x], value); returns what it held
// (the kernel: __hip_atomic_* at agent scope; the driver: std::atomic).
//
// The rules:
//  - every value label64[v] ever holds is the key of a sequence from which v is reachable.  It starts as v's own key;
//    umi_relax hands label64[u] down an edge u -> v (who reaches u reaches v); umi_jump hands v the label of the sequence its
//    label names (label64[v] = key[w], label64[w] = key[x]: x reaches w, w reaches v).  Every write is a fetch_min: values only
//    ever fall, and a write that comes late is refused by the minimum.
//  - at a fixpoint -- a full pass over the records in which nothing fell -- label64[v] <= label64[u] for every edge u -> v,
//    hence label64[v] <= label64[w] <= key[w] for every w that reaches v; with the rule above it IS the minimum of those
//    keys.  The fixpoint is one array, whatever the schedule of the passes that led to it.
//  - a pass hands every label at least one edge further (Bellman-Ford: after r passes label64[v] is at most the smallest key
//    within r edges of v, whatever the order inside a pass, because values only fall), and a shortest path has at most
//    n_u - 1 edges: pass n_u at the latest lowers nothing.  The host's loop is bounded by n_u + 1 launches, and nothing ever
//    waits for another thread.  The jumps can only shorten this.
#pragma once
#include <cstdint>

#include "hamming_step.h"

namespace sassy_hip {

SASSY_HAM_HD uint64_t umi_key(uint32_t count, uint32_t u) { return ((uint64_t)(0xFFFFFFFFu - count) << 32) | u; }
SASSY_HAM_HD uint32_t umi_key_index(uint64_t key) { return (uint32_t)key; }
// the edge u -> v between neighbours: c_u >= 2 c_v - 1 (two sequences of count 1 point at each other)
SASSY_HAM_HD bool umi_absorbs(uint32_t c_u, uint32_t c_v) { return (uint64_t)c_u + 1 >= 2 * (uint64_t)c_v; }

// label64[v] also takes the label of the sequence it names.  true: it fell.
template <typename M>
SASSY_HAM_HD bool umi_jump(M& mem, uint32_t v) {
  const uint64_t mine = mem.load(v);
  const uint32_t w = umi_key_index(mine);
  if (w == v) return false;
  const uint64_t far = mem.load(w);
  return far < mine && mem.fetch_min(v, far) > far;
}

// One neighbour pair {u, v}, u != v, with the two counts: each direction the count rule allows, then a jump at both ends.
// true: some label fell.
template <typename M>
SASSY_HAM_HD bool umi_relax(M& mem, uint32_t u, uint32_t v, uint32_t c_u, uint32_t c_v) {
  bool fell = false;
  const uint64_t lu = mem.load(u), lv = mem.load(v);
  if (umi_absorbs(c_u, c_v) && lu < lv) fell |= mem.fetch_min(v, lu) > lu;
  if (umi_absorbs(c_v, c_u) && lv < lu) fell |= mem.fetch_min(u, lv) > lv;
  fell |= umi_jump(mem, u);
  fell |= umi_jump(mem, v);
  return fell;
}

}  // namespace sassy_hip
