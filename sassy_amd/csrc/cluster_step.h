// cluster_step.h -- the union step of the clustering calls (clusters.hip: sassy_hip_hamming_clusters and
// sassy_hip_edit_clusters; DESIGN.md 5.10 "Clusters"), free of HIP and of the environment: plain C++17 that the link kernels
// (hamming_pairs.hip, edit_pairs.hip), the flatten kernel (clusters.hip) and the host test driver
// (tests/c/cluster_step_driver.cc) compile alike.
//
// A forest over the indices 0 .. n - 1 in one array, parent[x], that starts as parent[x] = x; x is a root while
// parent[x] == x.  The code is written against a memory policy M of two operations on that array, both relaxed:
//   uint32_t M::load(uint32_t x)                                   the value of parent[x]
//   bool     M::cas(uint32_t x, uint32_t expect, uint32_t desired)  parent[x] = desired if it still holds expect
// (the kernels: __hip_atomic_* at agent scope; the driver: std::atomic).  No operation needs an order beyond the coherence of
// one location: every value that parent[x] ever holds is a right one (below).
//
// The rules, which every function here keeps and every caller may rely on:
//  - parent[x] <= x always, and every write LOWERS a value: there is no plain store, every write is a compare-and-swap
//    from a value read before to a smaller one.  A chase x -> parent[x] -> ... therefore strictly descends and ends at a root
//    after at most n steps.  There is no cycle, so no chase can hang.
//  - every value written to parent[x] is an index of x's own tree: a root of it (cluster_link), an ancestor (cluster_find's
//    path splitting) or a node that was the tree's root earlier (cluster_lower).  Trees only ever merge, so a value that was
//    in x's tree once is in it for good -- which is why a write that comes late, behind other threads' writes, is harmless:
//    it still names a smaller index of the same tree, and the compare-and-swap refuses it unless it lowers what is there.
//  - two trees are joined by CAS(parent[hi], hi, lo) on ROOTS only, hi the larger of the two.  The smallest index of a
//    component can never get a parent (a parent is smaller and in the same component), so when all edges are linked each
//    component is one tree whose single root is its minimum -- the label, whatever the schedule.
//  - lock-free: the only loop that is not a descending chase is cluster_link's, and it goes round again only because its
//    CAS on a root failed, that is because another thread's link of that root SUCCEEDED -- at most n - 1 times in a whole
//    call.  No thread ever waits for another: no lock, no flag, no spin on a value some other lane of the wavefront has yet
//    to write (which under SIMT execution could never come).
#pragma once
#include <cstdint>

#include "hamming_step.h"

namespace sassy_hip {

// The root of x's tree as of some moment of the call.  Path splitting on the way: every node of the path is handed to its
// grandparent, by one compare-and-swap that is never tried again (it fails where another thread lowered the node first).
template <typename M>
SASSY_HAM_HD uint32_t cluster_find(M& mem, uint32_t x) {
  uint32_t p = mem.load(x);
  while (p != x) {
    const uint32_t g = mem.load(p);
    if (g != p) (void)mem.cas(x, p, g);
    x = p;
    p = g;
  }
  return x;
}

// Joins the trees of x and y; returns the root of the joined tree as of that moment (the smaller of the two roots).
template <typename M>
SASSY_HAM_HD uint32_t cluster_link(M& mem, uint32_t x, uint32_t y) {
  uint32_t rx = cluster_find(mem, x), ry = cluster_find(mem, y);
  while (rx != ry) {
    const uint32_t hi = rx > ry ? rx : ry, lo = rx > ry ? ry : rx;
    if (mem.cas(hi, hi, lo)) return lo;  // (lo may have got a parent meanwhile: hi still hangs in lo's tree)
    // hi is a root no longer -- another thread linked it: on from where both stand now
    rx = cluster_find(mem, hi);
    ry = cluster_find(mem, lo);
  }
  return rx;
}

// Hands x to v, an index that is or was the root of x's tree (v <= x), if that lowers parent[x]: one try.
template <typename M>
SASSY_HAM_HD void cluster_lower(M& mem, uint32_t x, uint32_t v) {
  const uint32_t p = mem.load(x);
  if (v < p) (void)mem.cas(x, p, v);
}

// What a link kernel does with a candidate pair {i, j}: `root` is the walking lane's register, the last root it knew of
// i's tree (i itself at the start).  Where j already hangs directly under it the two are joined and nothing else is read --
// the case that a dense set takes on all but a few of its hits; `root` may be stale there (a root no longer), it is in i's
// tree all the same.  Else the trees are linked and both ends handed to the new root, so that the next lane that looks at
// parent[j] or parent[i] finds it there.
template <typename M>
SASSY_HAM_HD void cluster_join(M& mem, uint32_t i, uint32_t j, uint32_t& root) {
  if (mem.load(j) == root) return;
  root = cluster_link(mem, root, j);
  cluster_lower(mem, j, root);
  cluster_lower(mem, i, root);
}

}  // namespace sassy_hip
