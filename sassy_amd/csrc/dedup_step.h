// dedup_step.h -- the arithmetic of deduplicating a resident read batch by UMI (dedup_reads.hip: sassy_hip_umi_groups_reads,
// sassy_hip_dedup_reads), free of HIP and of the environment: plain C++17 that the device kernels and the host test driver
// (tests/c/dedup_step_driver.cc) compile alike.  In the order of a call: what the call refuses, the key window of a read, the
// window as the pair family's bit planes (and its reverse complement's, for an rc searcher), the score of a read, the key
// whose maximum over a group names the kept read.
//
// Read r of la bytes; its key is the window of m <= 128 bytes at distance `at` from the chosen end (demux_step.h: dmx_window).
// The window is fetched as one 64-byte block for m <= 64 and two for m <= 128 (trim_step.h: trm_window_block, zero behind m)
// and packed into pairs_encode's planes: bit t of word t / 32 of plane p is bit p of pairs_row_code of byte t.  Here a plane
// is always four words in registers; the kernel stores the first pairs_words(m) of them at [p W + w].
#pragma once
#include <cstddef>
#include <cstdint>

#include "demux_step.h"

namespace sassy_hip {

constexpr uint32_t kDdpEnd3 = 1u;          // SASSY_HIP_DEDUP_END3
constexpr uint32_t kDdpMaxLen = 128;       // longest key: four words per plane (kPairsMaxRows)
constexpr uint32_t kDdpMaxMethod = 2;      // SASSY_HIP_UMI_DIRECTIONAL
constexpr uint32_t kDdpNone = 0xFFFFFFFFu; // label and rep of a read without a window
constexpr uint32_t kDdpScoreLanes = 8;     // lanes that share a read in the score kernel: 128 contiguous bytes a step

// ---- what the calls refuse, before any device work, in this order ----
struct DdpCall {
  bool have_searcher;
  uint32_t flags, method, at;
  size_t m;
  ReadsGate gate;                         // the searcher and the handle (reads_gate.h)
  bool have_out;                          // out_label (the groups call), out_dedup (the dedup call) != NULL
};
enum DdpRefusal : uint32_t { kDdpOk = 0, kDdpNullSearcher, kDdpFlags, kDdpMethod, kDdpLen, kDdpAt, kDdpGate /* *gate says which */, kDdpNullOut };
// The handle is read only once nothing in front of it is wrong.
inline DdpRefusal ddp_refusal(const DdpCall& c, ReadsRefusal* gate) {
  *gate = kRdsOk;
  if (!c.have_searcher) return kDdpNullSearcher;
  if (c.flags & ~kDdpEnd3) return kDdpFlags;
  if (c.method > kDdpMaxMethod) return kDdpMethod;
  if (c.m == 0 || c.m > kDdpMaxLen) return kDdpLen;
  if ((uint64_t)c.at + c.m > kOvlMaxLen) return kDdpAt;
  if ((*gate = reads_gate_searcher(c.gate)) != kRdsOk) return kDdpGate;
  if ((*gate = reads_gate_handles(c.gate)) != kRdsOk) return kDdpGate;
  if (!c.have_out) return kDdpNullOut;
  if ((*gate = reads_gate_tickets(c.gate)) != kRdsOk) return kDdpGate;
  return kDdpOk;
}

// ---- the planes of the window ----
SASSY_HAM_HD uint32_t ddp_bit_reverse(uint32_t x) {
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
  x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
  return (x >> 16) | (x << 16);
}
// word i of a four-word value, zero from 4 on (selects: the value stays in registers)
SASSY_HAM_HD uint32_t ddp_pick(const uint32_t (&v)[4], uint32_t i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : i == 3 ? v[3] : 0u; }
// rows 0 .. m - 1 of a plane, reversed: out bit t = in bit m - 1 - t, zero from m on.  The 128 bits reversed whole, then
// shifted down by 128 - m.
SASSY_HAM_HD void ddp_reverse_rows(const uint32_t (&in)[4], uint32_t m, uint32_t (&out)[4]) {
  const uint32_t rev[4] = {ddp_bit_reverse(in[3]), ddp_bit_reverse(in[2]), ddp_bit_reverse(in[1]), ddp_bit_reverse(in[0])};
  const uint32_t sh = kDdpMaxLen - m, q = sh >> 5, r = sh & 31u;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) out[w] = ovl_funnel(ddp_pick(rev, w + q), ddp_pick(rev, w + q + 1), r);
}
// One 64-byte block of the window (blk: sixteen words, zero behind the window) into words 2 b and 2 b + 1 of every plane:
// the forward planes, and -- RC -- the planes of the complemented bytes in the same order.
template <int P, bool RC, int B>
SASSY_HAM_HD void ddp_pack_block(uint32_t profile, const uint32_t (&blk)[16], uint32_t (&fw)[P][4], uint32_t (&cp)[P][4]) {
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    const uint32_t c = (blk[t >> 2] >> (8 * (t & 3))) & 0xFFu;
    const uint32_t code = pairs_row_code(profile, c);
#pragma unroll
    for (int p = 0; p < P; ++p) fw[p][2 * B + (t >> 5)] |= ((code >> p) & 1u) << (t & 31);
    if (RC) {
      const uint32_t comp = pairs_row_code(profile, ovl_complement(profile, c));
#pragma unroll
      for (int p = 0; p < P; ++p) cp[p][2 * B + (t >> 5)] |= ((comp >> p) & 1u) << (t & 31);
    }
  }
}
// block B of the window where the window reaches it (the same in every lane)
template <int P, bool RC, int B, typename Load16>
SASSY_HAM_HD void ddp_window_block(uint32_t profile, const Load16& load16, uint64_t src, uint64_t bytes, uint32_t m, uint32_t (&fw)[P][4],
                                   uint32_t (&cp)[P][4]) {
  if (64u * B >= m) return;
  uint32_t blk[16];
  trm_window_block(load16, src + 64u * B, bytes, m - 64u * B < 64u ? m - 64u * B : 64u, blk);
  ddp_pack_block<P, RC, B>(profile, blk, fw, cp);
}
// The window of m bytes at byte `src` of a buffer of `bytes` bytes (a multiple of 16; load16 as trm_window_block takes it):
// fw = pairs_encode of the window at four words a plane, rv -- RC -- pairs_encode of its reverse complement.  Rows from m
// on are zero in every plane whatever lies behind the window.
template <int P, bool RC, typename Load16>
SASSY_HAM_HD void ddp_window_planes(uint32_t profile, const Load16& load16, uint64_t src, uint64_t bytes, uint32_t m, uint32_t (&fw)[P][4],
                                    uint32_t (&rv)[P][4]) {
  uint32_t cp[P][4];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int w = 0; w < 4; ++w) fw[p][w] = cp[p][w] = rv[p][w] = 0u;
  ddp_window_block<P, RC, 0>(profile, load16, src, bytes, m, fw, cp);
  ddp_window_block<P, RC, 1>(profile, load16, src, bytes, m, fw, cp);
#pragma unroll
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {  // (byte 0 has a code of its own under neither profile; the mask says so)
      fw[p][w] &= pairs_row_mask(m, (uint32_t)w);
      cp[p][w] &= pairs_row_mask(m, (uint32_t)w);
    }
    if (RC) ddp_reverse_rows(cp[p], m, rv[p]);
  }
}

// ---- the score and the kept read ----
// the sum of the four bytes of a word
SASSY_HAM_HD uint32_t ddp_byte_sum(uint32_t w) {
  const uint32_t two = (w & 0x00FF00FFu) + ((w >> 8) & 0x00FF00FFu);
  return (two & 0xFFFFu) + (two >> 16);
}
// the bytes of 16-byte piece `piece` of a read of `len` bytes that are the read's: their sum (w: the piece's four words)
SASSY_HAM_HD uint32_t ddp_piece_sum(const uint32_t (&w)[4], uint32_t piece, uint32_t len) {
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t first = 16u * piece + 4u * j, left = len > first ? len - first : 0u;
    sum += ddp_byte_sum(left >= 4u ? w[j] : (w[j] & ((1u << (8u * left)) - 1u)));
  }
  return sum;
}
// pieces of a read of len bytes
SASSY_HAM_HD uint32_t ddp_pieces(uint32_t len) { return (len + 15u) >> 4; }
// The key of read r: the higher score wins, at equal scores the smaller index.  No read has the key 0 (r < 2^32 - 1), which
// is what a group's cell holds before its first read.
SASSY_HAM_HD uint64_t ddp_key(uint32_t score, uint32_t r) { return ((uint64_t)score << 32) | (0xFFFFFFFFu - r); }
SASSY_HAM_HD uint32_t ddp_key_read(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

}  // namespace sassy_hip
