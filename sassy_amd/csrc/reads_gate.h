// reads_gate.h -- what every call on a device-resident read batch refuses alike (read_overlaps, merge_pairs, trim_reads,
// demux_reads, umi_groups_reads, dedup_reads), free of HIP and of the environment: plain C++17 that the step
// headers, the host owner (reads_call.hip) and the host test drivers (tests/c/reads_gate_driver.cc and the steps' own)
// compile alike.  A call's own refusal function (ovl_refusal, trm_refusal, ...) walks its own checks and calls the two
// predicates here at their places: the searcher part behind the call's numbers, the handle part behind it -- with the call's
// own checks of the handles around it --, then the call's null outputs, then the tickets.  Also here: the length of a read
// as every kernel of the family takes it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "hamming_step.h"

namespace sassy_hip {

constexpr uint32_t kReadsMaxLen = 512;  // longest read of a batch these calls take (SASSY_HIP_OVERLAP_MAX_LEN)

// What a call reads off the searcher and off its one or two handles.
struct ReadsGate {
  uint32_t profile;                       // kHamDna, kHamIupac; anything else is an Ascii searcher
  bool overhang, only_best, max_n_frac;   // the searcher's reporting modes that are set
  uint32_t handles;                       // 1, or 2 for the pair calls
  bool have_reads[2];
  bool handle_read;                       // the fields below that come out of the handles are filled in
  int device_s, device_r[2];
  uint64_t longest[2];
  bool in_flight;                         // tickets are open on the searcher
};
enum ReadsRefusal : uint32_t { kRdsOk = 0, kRdsAscii, kRdsOverhang, kRdsOnlyBest, kRdsNFrac, kRdsNullReads, kRdsDevice, kRdsTooLong, kRdsInFlight };

// the searcher, then the handles as pointers
SASSY_HAM_HD ReadsRefusal reads_gate_searcher(const ReadsGate& g) {
  if (g.profile != kHamDna && g.profile != kHamIupac) return kRdsAscii;
  if (g.overhang) return kRdsOverhang;
  if (g.only_best) return kRdsOnlyBest;
  if (g.max_n_frac) return kRdsNFrac;
  for (uint32_t h = 0; h < g.handles; ++h)
    if (!g.have_reads[h]) return kRdsNullReads;
  return kRdsOk;
}
// what is read out of the handles, once they have been read: nothing in front of them was wrong
SASSY_HAM_HD ReadsRefusal reads_gate_handles(const ReadsGate& g) {
  if (!g.handle_read) return kRdsOk;
  for (uint32_t h = 0; h < g.handles; ++h)
    if (g.device_r[h] != g.device_s) return kRdsDevice;
  for (uint32_t h = 0; h < g.handles; ++h)
    if (g.longest[h] > kReadsMaxLen) return kRdsTooLong;
  return kRdsOk;
}
SASSY_HAM_HD ReadsRefusal reads_gate_tickets(const ReadsGate& g) { return g.in_flight ? kRdsInFlight : kRdsOk; }

// The length of a read as the kernels take it: the host refused reads longer than max_len; a read that does not fit its
// text (start, len: the handle's table; bytes: its text size) counts as empty.
SASSY_HAM_HD uint32_t reads_fit_len(uint64_t start, uint64_t len, uint64_t bytes, uint64_t max_len) {
  const bool fits = len <= max_len && start <= bytes && len <= bytes - start;
  return fits ? (uint32_t)len : 0u;
}

}  // namespace sassy_hip
