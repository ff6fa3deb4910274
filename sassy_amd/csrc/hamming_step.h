// hamming_step.h -- the arithmetic of the Hamming search (hamming.hip), free of HIP: plain C++17 that the device kernels and
// the host test drivers (tests/c/hamming_step_driver.cc, hamming_many_step_driver.cc, hamming_counts_step_driver.cc) compile alike.
//
// H(s) = #{ j < m : !match(P[j], T[s + j]) }.  The text comes as slot masks: per 64-byte block b and profile slot c one
// 64-bit word, bit i = "text byte 64 b + i matches slot c".  Row j of the pattern names its slot.  For the 64 starts of one
// block, row j's match bits are the 64-bit window at bit offset j of the row's slot masks of the blocks from b on, so a
// block needs the masks of the W = ceil((m - 1) / 64) blocks to its right.  The mismatches are counted in bit-sliced
// counters: plane p holds bit p of all 64 counts, a carry out of the top plane sticks in `over` (the count saturates).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SASSY_HAM_HD __host__ __device__ __forceinline__
#else
#define SASSY_HAM_HD inline
#endif

namespace sassy_hip {

constexpr uint32_t kHamMaxRows = 1024;   // longest pattern: W <= 16 halo blocks
constexpr uint32_t kHamTileBlocks = 64;  // blocks a wavefront owns: one per lane
constexpr uint32_t kHamMaxHalo = 16;     // = ham_halo_blocks(kHamMaxRows)
constexpr int kHamNPlanes = 11;          // counter planes of the N count (<= m <= 1024 < 2^11)

SASSY_HAM_HD uint32_t ham_halo_blocks(uint32_t m) { return (m - 1 + 63) / 64; }
// counter planes for threshold k (k <= m <= kHamMaxRows): the smallest of 2, 4, 8, 11 with k < 2^planes
SASSY_HAM_HD int ham_planes(uint32_t k) { return k < 4 ? 2 : k < 16 ? 4 : k < 256 ? 8 : 11; }

// bits [sh, sh + 64) of the 128-bit word b:a, 0 <= sh < 64
SASSY_HAM_HD uint64_t ham_window(uint64_t a, uint64_t b, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t w0 = (uint32_t)a, w1 = (uint32_t)(a >> 32), w2 = (uint32_t)b, w3 = (uint32_t)(b >> 32);
  if (sh & 32u) { w0 = w1; w1 = w2; w2 = w3; }  // (sh is wave-uniform)
  const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh & 31u), hi = __builtin_amdgcn_alignbit(w2, w1, sh & 31u);
  return ((uint64_t)hi << 32) | lo;
#else
  return (a >> sh) | ((b << 1) << (63u - sh));
#endif
}

// P planes count 0 .. 2^P - 1; beyond that `over` is set and stays set
template <int P>
struct HamCounter {
  uint64_t c[P];
  uint64_t over;
  SASSY_HAM_HD void clear() {
#pragma unroll
    for (int p = 0; p < P; ++p) c[p] = 0;
    over = 0;
  }
  SASSY_HAM_HD void add(uint64_t x) {  // ripple: plane p takes the carry of plane p - 1
    uint64_t carry = x;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const uint64_t t = c[p] & carry;
      c[p] ^= carry;
      carry = t;
    }
    over |= carry;
  }
  // bit i: count i <= k
  SASSY_HAM_HD uint64_t le(uint32_t k) const {
    if (k >= (1u << P) - 1u) return ~over;
    uint64_t gt = 0, eq = ~(uint64_t)0;
#pragma unroll
    for (int p = P - 1; p >= 0; --p) {
      if ((k >> p) & 1u) {
        eq &= c[p];
      } else {
        gt |= eq & c[p];
        eq &= ~c[p];
      }
    }
    return ~gt & ~over;
  }
  // bit i: count i == v, for v < 2^P; a start with `over` set never matches.  A start that survives le(k) did not saturate,
  // so its planes hold its exact count: eq(v) & hit is exact for every v <= k, and the eq(v), v <= k, partition le(k).
  SASSY_HAM_HD uint64_t eq(uint32_t v) const {
    uint64_t e = ~over;
#pragma unroll
    for (int p = 0; p < P; ++p) e &= ((v >> p) & 1u) ? c[p] : ~c[p];
    return e;
  }
};

// The 64 starts of one block: bit i = "at most k of the m rows mismatch at start 64 b + i" (invert = true), or, with
// invert = false, "at most k of the m rows hit" (the N count: one slot, whose mask marks the N).
//   fetch(slot, q)  the slot's mask of block b + q, 0 <= q <= ham_halo_blocks(m)
//   row_word(w)     the slots of rows 4w .. 4w + 3, one byte each, row 4w in the low byte
//   all_over(over)  may the loop stop: true only if no start of any block that shares this loop can still pass
//                   (one block: over == ~0; a wavefront: a vote over its lanes)
//   cnt             the counter planes as the loop leaves them (stopped early: over == ~0 in every block of the loop)
template <int P, bool INVERT, typename Fetch, typename RowWord, typename AllOver>
SASSY_HAM_HD void ham_count(const Fetch& fetch, const RowWord& row_word, uint32_t m, const AllOver& all_over, HamCounter<P>& cnt) {
  cnt.clear();
  const uint32_t nw = (m + 3) / 4;
  for (uint32_t w = 0; w < nw; ++w) {
    const uint32_t slots = row_word(w);
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t j = 4 * w + r;
      if (j < m) {
        const uint32_t slot = (slots >> (8 * r)) & 0xFFu, q = j >> 6, sh = j & 63u;
        const uint64_t a = fetch(slot, q);
        const uint64_t b = sh ? fetch(slot, q + 1) : 0;  // (q + 1 <= W whenever sh != 0)
        const uint64_t win = ham_window(a, b, sh);
        cnt.add(INVERT ? ~win : win);
      }
    }
    if (all_over(cnt.over)) break;
  }
}
template <int P, bool INVERT, typename Fetch, typename RowWord, typename AllOver>
SASSY_HAM_HD uint64_t ham_hit_mask(const Fetch& fetch, const RowWord& row_word, uint32_t m, uint32_t k, const AllOver& all_over) {
  HamCounter<P> cnt;
  ham_count<P, INVERT>(fetch, row_word, m, all_over, cnt);
  return cnt.le(k);
}

// The smallest count among the starts of `hit` (a subset of the starts whose count did not saturate) and, in *at, the starts
// that attain it: the planes narrow the candidates from the top -- where some candidate has a 0 in plane p, the minimum has,
// and only those stay.  P steps, no count is extracted per start.  hit == 0 (after ~over): 0xFFFFFFFF, *at = 0.
template <int P>
SASSY_HAM_HD uint32_t ham_min_cost(const HamCounter<P>& cnt, uint64_t hit, uint64_t* at) {
  uint64_t cand = hit & ~cnt.over;
  *at = cand;
  if (cand == 0) return 0xFFFFFFFFu;
  uint32_t cost = 0;
#pragma unroll
  for (int p = P - 1; p >= 0; --p) {
    const uint64_t t = cand & ~cnt.c[p];
    if (t) cand = t;
    else cost |= 1u << p;
  }
  *at = cand;
  return cost;
}
// The largest count among the starts of `hit`, the mirror image: where some candidate has a 1 in plane p, the maximum has.
// hit == 0 (after ~over): 0 -- a caller that has to tell "none" from "all zero" asks ham_min_cost.  With the minimum it bounds
// the costs a block's hits can have (hamming_counts: the wavefront's loop over costs).
template <int P>
SASSY_HAM_HD uint32_t ham_max_cost(const HamCounter<P>& cnt, uint64_t hit) {
  uint64_t cand = hit & ~cnt.over;
  if (cand == 0) return 0;
  uint32_t cost = 0;
#pragma unroll
  for (int p = P - 1; p >= 0; --p) {
    const uint64_t t = cand & cnt.c[p];
    if (t) {
      cand = t;
      cost |= 1u << p;
    }
  }
  return cost;
}

// starts of block b that lie in the text: 64 b + i + m <= n.  By position -- no byte value excludes a start.
SASSY_HAM_HD uint64_t ham_valid_mask(uint64_t block, uint64_t n, uint32_t m) {
  if (n < m) return 0;
  const uint64_t last = n - m, s0 = block * 64;
  if (s0 > last) return 0;
  if (last - s0 >= 63) return ~(uint64_t)0;
  return ((uint64_t)2 << (last - s0)) - 1;
}

// ---- a batch of texts in one buffer, each from a multiple of 64 bytes on (search_hamming_many) ----
// bytes from the first byte of block `block` to the end of the text [start, start + len) it lies in, saturated
SASSY_HAM_HD uint32_t ham_rem(uint64_t block, uint64_t start, uint64_t len) {
  const uint64_t end = start + len, s0 = block * 64;
  if (end <= s0) return 0;
  return end - s0 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(end - s0);
}
// starts of a block that lie in the block's own text: i + m <= rem.  By position, as ham_valid_mask: the halo blocks may hold
// the next text, and a start whose window reaches them is dropped whatever they hold.
SASSY_HAM_HD uint64_t ham_valid_mask_rem(uint32_t rem, uint32_t m) {
  if (rem < m) return 0;
  const uint32_t last = rem - m;
  if (last >= 63) return ~(uint64_t)0;
  return ((uint64_t)2 << last) - 1;
}
// The text that byte `pos` of the buffer lies in: the last t < n_texts with start(t) <= pos (start ascends, start(0) == 0).  An
// empty text takes no block and shares its start with the text behind it, so the last of a run of equal starts is the one
// that owns the bytes; empty texts at the buffer's end start at its size, behind every block.
template <typename Start>
SASSY_HAM_HD uint32_t ham_text_of(const Start& start, uint32_t n_texts, uint64_t pos) {
  uint32_t lo = 0, hi = n_texts;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (start(mid) <= pos) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- the relation, per byte (the emit kernel; profiles.h: scan_eq) ----
constexpr uint32_t kHamDna = 1, kHamIupac = 2, kHamAsciiCi = 4;  // = Profile (common.h); anything else: byte equality
// IUPAC letter (c & 31) -> its base set, A=1 C=2 T=4 G=8; what is no letter acts as N, X is the empty set
SASSY_HAM_HD uint32_t ham_iupac_nib(uint32_t c) {
  switch (c & 31u) {
    case 1: return 1;    // A
    case 2: return 14;   // B
    case 3: return 2;    // C
    case 4: return 13;   // D
    case 7: return 8;    // G
    case 8: return 7;    // H
    case 11: return 12;  // K
    case 13: return 3;   // M
    case 18: return 9;   // R
    case 19: return 10;  // S
    case 20: return 4;   // T
    case 21: return 4;   // U
    case 22: return 11;  // V
    case 23: return 5;   // W
    case 24: return 0;   // X
    case 25: return 6;   // Y
    default: return 15;
  }
}
SASSY_HAM_HD uint32_t ham_fold(uint32_t c) { return (c | 0x20u) - 'a' < 26u ? (c | 0x20u) : c; }
SASSY_HAM_HD bool ham_match(uint32_t profile, uint32_t p, uint32_t t) {
  if (profile == kHamDna) return ((p >> 1) & 3u) == ((t >> 1) & 3u);
  if (profile == kHamIupac) return (ham_iupac_nib(p) & ham_iupac_nib(t)) != 0;
  if (profile == kHamAsciiCi) return ham_fold(p) == ham_fold(t);
  return p == t;
}
SASSY_HAM_HD bool ham_is_n(uint32_t t) { return (t | 0x20u) == 0x6Eu; }

// One hit: cost, N count and the run-length cigar ('=' / 'X') of the m window bytes text(0 .. m - 1) against pat[0 .. m),
// the pattern as it was scanned.  minus: pat is the reverse complement of the caller's pattern, and the cigar runs in the
// caller's pattern direction -- from the window's last byte to its first.  cigar == nullptr: no cigar.  The cigar takes at
// most 2 m bytes and a NUL.
template <typename Text>
SASSY_HAM_HD void ham_emit_hit(uint32_t profile, const uint8_t* pat, uint32_t m, const Text& text, bool minus, char* cigar,
                               uint32_t* cost, uint32_t* n_count, uint32_t* cigar_len) {
  uint32_t c = 0, nn = 0, len = 0, run = 0;
  char op = 0;
  auto flush = [&]() {
    if (!cigar || run == 0) return;
    char digits[10];
    int nd = 0;
    for (uint32_t v = run; v; v /= 10) digits[nd++] = (char)('0' + v % 10);
    while (nd) cigar[len++] = digits[--nd];
    cigar[len++] = op;
  };
  for (uint32_t j = 0; j < m; ++j) {
    const uint32_t i = minus ? m - 1 - j : j;
    const uint32_t t = text(i);
    const bool eq = ham_match(profile, pat[i], t);
    c += eq ? 0u : 1u;
    nn += ham_is_n(t) ? 1u : 0u;
    const char o = eq ? '=' : 'X';
    if (o != op) {
      flush();
      op = o;
      run = 0;
    }
    ++run;
  }
  flush();
  if (cigar) cigar[len] = 0;
  *cost = c;
  *n_count = nn;
  *cigar_len = len;
}

// The N filter's threshold (the reference's traced-span rule): the largest count c <= m with float(c) / float(m) <= frac,
// -1 if not even 0 passes; c == m: the filter drops nothing.
inline int64_t ham_n_max(uint32_t m, float max_n_frac) {
  int64_t best = -1;
  for (uint32_t c = 0; c <= m; ++c)
    if ((float)c / (float)m <= max_n_frac) best = c;
    else break;
  return best;
}

}  // namespace sassy_hip
