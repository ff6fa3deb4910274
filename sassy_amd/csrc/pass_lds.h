// The LDS layout of one wave of the shared pass's fused launches (scan_driver.hip: ScanJob::enqueue_pass sizes the launch;
// scan_kernel.hip: filter_dna_kernel<.., G, SRC> addresses it).  Plain C++, no HIP: (members, source, queue capacity) in,
// byte ranges out, so that host and kernel cannot disagree and the layout is checked on the CPU
// (tests/test_pass_lds_cpu.py).
//
// A wave's bytes, front to back:
//   dp      the chunk DP's slot masks (four of 512 bytes) and the carries of at most kPassLdsMaxWords pattern words (512
//           bytes each; the one-member staging launch, which lone searches use too: twelve such rows).  In a launch
//           that stages text the same bytes are the text tile while the wave streams.
//   state   what a segment leaves for the next while the DP runs: [7][64] u32 for one member, [11][64] for two.
//   queue   per member: `cap` chunk entries of 8 bytes, then the count (16 bytes).
// Launches that stage text (kPlaneRaw, kPlaneWrite) stream through a tile of 8 192 bytes: the state lies inside the tile's
// upper half, the queues behind the tile.  A launch that reads kept planes (kPlaneRead) stages nothing: its queues follow
// the state at once, and four workgroups of two members share a CU's 160 KiB.
#pragma once
#include <cstdint>

#include "plane_cache.h"  // (kPlaneRaw / kPlaneWrite / kPlaneRead)

namespace sassy_hip {

constexpr uint32_t kPassLdsTile = 64 * 128;    // the staging tile of one wave (common.h: kTileBytes)
constexpr uint32_t kPassLdsDpSlots = 4;        // slot masks of the chunk DP (filter_dna_kernel's DPNS in these launches)
constexpr uint32_t kPassLdsMaxWords = 4;       // pattern words per member (common.h: kFuseGroupMaxWords)
constexpr uint32_t kPassLdsWaves = 4;          // waves per workgroup (common.h: kWavesPerGroup)
constexpr uint32_t kPassLdsCuBytes = 160 * 1024;
constexpr uint32_t kPassLdsQueueCap = 192;     // chunk entries per queue the fused launches ask for (ScanJob::prepare)

struct LdsRange {
  uint32_t begin, end;  // bytes from the wave's base: [begin, end)
};

// the chunk DP's masks and carries (text-staging launches: the tile's lower part while the DP runs).  Four masks and the
// carries of kPassLdsMaxWords words; the one-member staging launch is also the lone search's, whose DP has up to eight
// masks or eight pattern words: twelve rows of 512 bytes.
constexpr LdsRange pass_lds_dp(int members, int src) {
  return LdsRange{0u, (members == 2 || src == kPlaneRead ? kPassLdsDpSlots + kPassLdsMaxWords : 12u) * 512u};
}
// the saved segment state: rows of 64 u32
constexpr uint32_t pass_lds_state_rows(int members) { return members == 2 ? 11u : 7u; }
constexpr LdsRange pass_lds_state(int members, int src) {
  const uint32_t at = pass_lds_dp(members, src).end;  // 4096, or 6144 in the one-member staging launch
  return LdsRange{at, at + pass_lds_state_rows(members) * 256u};
}
// where the queues begin: behind the tile, or -- nothing staged -- behind the state
constexpr uint32_t pass_lds_queues(int members, int src) { return src == kPlaneRead ? pass_lds_state(members, src).end : kPassLdsTile; }
constexpr uint32_t pass_lds_queue_stride(uint32_t cap) { return cap * 8u + 16u; }
// member g's chunk queue and, behind it, its count
constexpr LdsRange pass_lds_queue(int members, int src, uint32_t cap, int g) {
  const uint32_t at = pass_lds_queues(members, src) + (uint32_t)g * pass_lds_queue_stride(cap);
  return LdsRange{at, at + cap * 8u};
}
constexpr LdsRange pass_lds_count(int members, int src, uint32_t cap, int g) {
  const uint32_t at = pass_lds_queue(members, src, cap, g).end;
  return LdsRange{at, at + 16u};
}
constexpr uint32_t pass_lds_per_wave(int members, int src, uint32_t cap) {
  return pass_lds_queues(members, src) + (uint32_t)members * pass_lds_queue_stride(cap);
}
// the two-member launches' piece-row table: static LDS in front of the launch's own (piece_pair_step.h)
constexpr uint32_t pass_lds_table(int members, int q) { return members == 2 ? (uint32_t)q * 64u : 0u; }
constexpr uint32_t pass_lds_per_group(int members, int src, uint32_t cap, int q) {
  return kPassLdsWaves * pass_lds_per_wave(members, src, cap) + pass_lds_table(members, q);
}

}  // namespace sassy_hip
