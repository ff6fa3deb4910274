// pairs_step.h -- the arithmetic of the all-vs-all Hamming calls (hamming_pairs.hip: sassy_hip_hamming_pairs and
// sassy_hip_hamming_nearest), free of HIP and of the environment: plain C++17 that the device kernels and the host test driver
// (tests/c/pairs_step_driver.cc) compile alike.  In the order of a call: the bit-plane encoding of a sequence, the distance of
// two encoded sequences word by word, the combine rule of the partial cells, the plan -- strips of A, chunks of B, the tiles a
// self-mode call skips.
//
// Two lists of sequences of one length m <= 128, H(x, y) = #{ t < m : !match(x[t], y[t]) } under the profile relation of the
// family (hamming_step.h: ham_match).  A sequence becomes P bit planes of W 32-bit words, bit t of word t / 32 of plane p
// telling one thing about row t:
//   Dna    P = 2: bit p of the code (c >> 1) & 3                      mismatch word = OR_p (a_p ^ b_p)
//   Ascii  P = 8: bit p of the byte (ascii_ci: of the folded byte)    mismatch word = OR_p (a_p ^ b_p)
//   Iupac  P = 4: base p (A, C, T, G) is in the letter's set          match word    = OR_p (a_p & b_p)
// The kernels exist for W in {1, 2, 4}; a sequence is encoded at the next of these and its higher words are zero.  Pad bits
// (rows m .. 32 W - 1) are zero in every plane: under xor they never mismatch; under Iupac the mismatch word is the complement
// of the match word under the row mask of the word, so that they count as neither.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "hamming_step.h"

namespace sassy_hip {

constexpr uint32_t kPairsMaxRows = 128;    // longest sequence: 4 words per plane
constexpr uint32_t kPairsStrip = 256;      // A entries of a workgroup: one per lane
constexpr uint32_t kPairsWave = 64;        // A entries of a tile (a wavefront)
constexpr uint32_t kPairsMaxChunks = 65535;  // chunks of B: the grid's second dimension

SASSY_HAM_HD uint32_t pairs_planes(uint32_t profile) { return profile == kHamDna ? 2u : profile == kHamIupac ? 4u : 8u; }
// words per plane the kernel is instantiated for: 1, 2 or 4 (m <= 128)
SASSY_HAM_HD uint32_t pairs_words(uint32_t m) { return m <= 32 ? 1u : m <= 64 ? 2u : 4u; }
// the rows of word w of a sequence of m rows, as a mask
SASSY_HAM_HD uint32_t pairs_row_mask(uint32_t m, uint32_t w) {
  return m >= 32 * (w + 1) ? 0xFFFFFFFFu : m <= 32 * w ? 0u : (1u << (m - 32 * w)) - 1u;
}
// what the planes of one row say: plane p's bit is bit p of this value
SASSY_HAM_HD uint32_t pairs_row_code(uint32_t profile, uint32_t c) {
  if (profile == kHamDna) return (c >> 1) & 3u;
  if (profile == kHamIupac) return ham_iupac_nib(c) & 15u;
  return profile == kHamAsciiCi ? ham_fold(c) : c;
}
// out[p * W + w], P * W words: the planes of seq[0 .. m), W = pairs_words(m) or larger
inline void pairs_encode(uint32_t profile, const uint8_t* seq, uint32_t m, uint32_t W, uint32_t* out) {
  const uint32_t P = pairs_planes(profile);
  std::fill(out, out + P * W, 0u);
  for (uint32_t t = 0; t < m; ++t) {
    const uint32_t code = pairs_row_code(profile, seq[t]);
    for (uint32_t p = 0; p < P; ++p) out[p * W + (t >> 5)] |= ((code >> p) & 1u) << (t & 31u);
  }
}
// the reverse complement of seq[0 .. m) as the family scans it: complement(byte) is the profile's (profiles.h: complement_char)
template <typename Complement>
inline void pairs_reverse_complement(const uint8_t* seq, uint32_t m, const Complement& complement, uint8_t* out) {
  for (uint32_t t = 0; t < m; ++t) out[t] = complement(seq[m - 1 - t]);
}

// popcount that accumulates (the kernels: v_bcnt_u32_b32 with its accumulate operand)
SASSY_HAM_HD uint32_t pairs_popcount(uint32_t x, uint32_t acc) { return (uint32_t)__builtin_popcount(x) + acc; }
// The mismatching rows of word w.  a, b: the planes of the two sequences, plane p's word at [p * W + w]; mask: pairs_row_mask
// (read by Iupac only).
template <int P, int W, bool IUPAC>
SASSY_HAM_HD uint32_t pairs_mismatch_word(const uint32_t* a, const uint32_t* b, int w, uint32_t mask) {
  uint32_t acc = 0;
#pragma unroll
  for (int p = 0; p < P; ++p) acc |= IUPAC ? (a[p * W + w] & b[p * W + w]) : (a[p * W + w] ^ b[p * W + w]);
  return IUPAC ? ~acc & mask : acc;
}
// H of two encoded sequences of m rows
template <int P, int W, bool IUPAC>
SASSY_HAM_HD uint32_t pairs_cost(const uint32_t* a, const uint32_t* b, uint32_t m) {
  uint32_t cost = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) cost = pairs_popcount(pairs_mismatch_word<P, W, IUPAC>(a, b, w, IUPAC ? pairs_row_mask(m, (uint32_t)w) : 0u), cost);
  return cost;
}
// ---- partial cells ----
// What one A entry has seen of a run of target records r = S j + strand (S = 2 for an rc searcher, else 1), walked in
// ascending r: the candidates with cost <= k, the smallest key (cost, r) among them, how many share that smallest cost.
struct PairsCell {
  uint32_t cost;    // kPairsNoCost: no candidate
  uint32_t r;       // the first record at that cost
  uint32_t ties;    // candidates at that cost; the row pass of hamming_pairs keeps the cell's first record's place in its row here
  uint32_t n_hits;  // candidates
};
constexpr uint32_t kPairsNoCost = 0xFFFFFFFFu;
SASSY_HAM_HD PairsCell pairs_empty_cell() { return PairsCell{kPairsNoCost, 0xFFFFFFFFu, 0u, 0u}; }
// `a` then `b`, every record of b behind every record of a: the cell of the two runs together.  One candidate is a cell
// {cost, r, 1, 1}; a sequential walk is this rule applied per candidate.
SASSY_HAM_HD PairsCell pairs_combine(const PairsCell& a, const PairsCell& b) {
  PairsCell c = a;
  c.n_hits += b.n_hits;
  if (b.cost < a.cost) {
    c.cost = b.cost; c.r = b.r; c.ties = b.ties;
  } else if (b.cost == a.cost) {
    c.ties += b.ties;
  }
  return c;
}

// ---- the plan ----
// which (i, j, strand) a call visits: all of them; the triangle of self-mode pairs (strand 0: j > i, strand 1: j >= i); the
// square of self-mode nearest without (i, i, 0)
constexpr uint32_t kPairsCross = 0, kPairsSelfPairs = 1, kPairsSelfNearest = 2;
SASSY_HAM_HD bool pairs_visits(uint32_t mode, uint64_t i, uint64_t j, uint32_t strand) {
  if (mode == kPairsSelfPairs) return strand ? j >= i : j > i;
  if (mode == kPairsSelfNearest) return j != i || strand != 0;
  return true;
}
// Strips of kPairsStrip A entries x chunks of `chunk` targets (both strands of a target in one chunk); a tile is one
// wavefront's kPairsWave entries against one chunk.
struct PairsPlan {
  uint64_t n_a = 0, n_b = 0;
  uint32_t mode = kPairsCross;
  uint64_t n_strips = 0;
  uint32_t n_chunks = 0;
  uint64_t chunk = 0;  // targets per chunk (the last may hold fewer)
};
// How many chunks: forced > 0 that many (option pairs_chunks), else enough that `want_groups` workgroups are in flight, each
// chunk at least kPairsStrip targets where there are that many -- a large A fills the device alone.  fine_chunk > 0
// (hamming_pairs): also enough that a chunk holds at most that many targets, as the fill pass walks again every (wavefront,
// chunk) tile that holds a record.  Either way the partials matrix holds at most `max_cells` cells.  Never more chunks than
// targets, never more than kPairsMaxChunks.
constexpr uint64_t kPairsFineChunk = 16384;
inline PairsPlan pairs_plan(uint64_t n_a, uint64_t n_b, uint32_t mode, long forced, uint64_t fine_chunk = 0, uint64_t want_groups = 2048,
                            uint64_t max_cells = 1ull << 24) {
  PairsPlan p;
  p.n_a = n_a; p.n_b = n_b; p.mode = mode;
  p.n_strips = (n_a + kPairsStrip - 1) / kPairsStrip;
  uint64_t chunks;
  if (forced > 0) {
    chunks = (uint64_t)forced;
  } else {
    chunks = (want_groups + p.n_strips - 1) / p.n_strips;
    chunks = std::min(chunks, std::max<uint64_t>(1, n_b / kPairsStrip));
    if (fine_chunk > 0) chunks = std::max(chunks, (n_b + fine_chunk - 1) / fine_chunk);
    chunks = std::min(chunks, std::max<uint64_t>(1, max_cells / std::max<uint64_t>(1, n_a)));
  }
  chunks = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(chunks, n_b), kPairsMaxChunks));
  p.chunk = (n_b + chunks - 1) / chunks;
  p.n_chunks = (uint32_t)((n_b + p.chunk - 1) / p.chunk);  // (no empty chunk at the end)
  return p;
}
// the targets of chunk c
SASSY_HAM_HD uint64_t pairs_chunk_begin(uint64_t chunk, uint64_t c) { return chunk * c; }
SASSY_HAM_HD uint64_t pairs_chunk_end(uint64_t chunk, uint64_t n_b, uint64_t c) { return chunk * (c + 1) < n_b ? chunk * (c + 1) : n_b; }
// Where the tile of entries [i0, i0 + kPairsWave) starts its walk of targets [j0, j1): self-mode pairs never visit j < i, so
// a tile that lies wholly below the diagonal is skipped (the walk is empty) and one on it starts at its first entry.
SASSY_HAM_HD uint64_t pairs_tile_first(uint32_t mode, uint64_t i0, uint64_t j0, uint64_t j1) {
  if (mode != kPairsSelfPairs || i0 <= j0) return j0;
  return i0 < j1 ? i0 : j1;
}

}  // namespace sassy_hip
