// collapse_step.h -- the duplicate table of the UMI grouping call (umi_groups.hip: sassy_hip_umi_groups; DESIGN.md 5.10 "UMI
// groups"), free of HIP and of the environment: plain C++17 that the collapse kernels and the host test driver
// (tests/c/collapse_step_driver.cc) compile alike.
//
// n entries, each with a key (the call: the entry's plane words); two entries are duplicates when their keys are equal.  The
// answer wanted is, per entry, the SMALLEST index among its duplicates.  One open-addressing table of n_slots >= n 32-bit
// slots that start as kCollapseEmpty; an entry's probes start at slot h % n_slots, h a hash of its key, and go on slot by slot,
// wrapping round.  The code is written against a memory policy M of three operations on the table, all relaxed:
//   uint32_t M::load(uint64_t slot)                                       the slot's value
//   uint32_t M::cas(uint64_t slot, uint32_t expect, uint32_t desired)      slot = desired if it holds expect; returns what it
//                                                                         held (== expect: the swap was made)
//   uint32_t M::fetch_min(uint64_t slot, uint32_t value)                   slot = min(slot, value); returns what it held
// (the kernels: __hip_atomic_* at agent scope; the driver: std::atomic) and a predicate same(v): entry v's key equals the
// inserting entry's.  Keys are read-only for the whole call.
//
// The rules, which both functions keep and every caller may rely on:
//  - a slot leaves EMPTY once, by the compare-and-swap of the entry that claims it, and never returns to it; from then on
//    it holds indices of ONE class of duplicates only -- the claimer's: every later write is a fetch_min by an entry that has
//    seen an index of its own class there.  A slot's class is fixed at its claim, its value only ever falls.
//  - the entries of one class all end at the same slot: the first slot of their common probe sequence that their class owns.
//    None of them can pass it (they find an equal key there), none can stop earlier (an earlier slot is owned by another
//    class, or was EMPTY and the entry's own claim would have made it the class's slot).  After all inserts that slot holds
//    the minimum of the class, whatever the schedule and whatever the hash: the hash decides where a class lives, never what
//    its slot holds.
//  - a class takes one slot, so a table of n_slots >= n never runs out: an insert ends within n_slots probes, also at load 1.
//  - no entry waits for a value another entry has yet to write.  A failed compare-and-swap means the slot NOW holds an index --
//    the value the operation returned -- and the entry goes on with that value: compares keys, merges or steps to the next slot.
//    There is no spin, so no livelock where the lanes of a wavefront run in lock step.
//  - the plain look comes first: where the slot already holds an index <= i of i's class nothing is written, so a million
//    identical entries do not queue on one address -- only those that lower the slot pay for an atomic.
#pragma once
#include <cstddef>
#include <cstdint>

#include "hamming_step.h"

namespace sassy_hip {

constexpr uint32_t kCollapseEmpty = 0xFFFFFFFFu;

// a hash of n_words 32-bit words (the answer of the call does not depend on it: collapse_slots_for and the rules above)
SASSY_HAM_HD uint32_t collapse_hash(const uint32_t* words, uint32_t n_words) {
  uint32_t h = 0x9E3779B9u;
  for (uint32_t q = 0; q < n_words; ++q) {
    h ^= words[q];
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
  }
  return h;
}

// slots of the table for n entries: forced > 0 (option collapse_slots) that many but at least n, else the power of two that
// is at least 2 n
inline uint64_t collapse_slots_for(uint64_t n, long forced) {
  if (forced > 0) return (uint64_t)forced < n ? n : (uint64_t)forced;
  uint64_t slots = 2;
  while (slots < 2 * n) slots <<= 1;
  return slots;
}

// Entry i into the table.  false: n_slots probes and no slot -- more classes than slots, which n_slots >= n rules out.
template <typename M, typename Same>
SASSY_HAM_HD bool collapse_insert(M& mem, uint64_t n_slots, uint32_t h, uint32_t i, Same&& same) {
  uint64_t slot = (uint64_t)h % n_slots;
  for (uint64_t probe = 0; probe < n_slots; ++probe) {
    uint32_t v = mem.load(slot);
    if (v == kCollapseEmpty) {
      v = mem.cas(slot, kCollapseEmpty, i);
      if (v == kCollapseEmpty) return true;  // claimed: the slot is i's class's
      // (else another entry claimed it first: v is that index now, no wait)
    }
    if (v == i || same(v)) {
      if (v > i) (void)mem.fetch_min(slot, i);  // (v <= i: the slot holds an index of the class that is no worse)
      return true;
    }
    slot = slot + 1 == n_slots ? 0 : slot + 1;
  }
  return false;
}

// After every insert is done: the smallest duplicate of entry i -- the value of its class's slot.  kCollapseEmpty: i was
// never inserted.
template <typename M, typename Same>
SASSY_HAM_HD uint32_t collapse_lookup(M& mem, uint64_t n_slots, uint32_t h, uint32_t i, Same&& same) {
  uint64_t slot = (uint64_t)h % n_slots;
  for (uint64_t probe = 0; probe < n_slots; ++probe) {
    const uint32_t v = mem.load(slot);
    if (v == kCollapseEmpty) return kCollapseEmpty;
    if (v == i || same(v)) return v;
    slot = slot + 1 == n_slots ? 0 : slot + 1;
  }
  return kCollapseEmpty;
}

}  // namespace sassy_hip
