// amplicon_step.h -- the arithmetic of the amplicon join (amplicons.hip), free of HIP: plain C++17 that the device kernels and
// the host test driver (tests/c/amplicon_step_driver.cc) compile alike.
//
// The Hamming scan leaves, per scanned pattern, a run of items sorted by block: (block, 64-bit mask), bit i = "start
// 64 block + i is a hit"; blocks without a hit have no item.  A LEFT hit at s (the primer that sits on the forward strand at
// the product's start) joins with every PARTNER hit (the other primer's reverse complement, of length b_partner) whose start
// lies in the window that the product's length allows.  Everything here works on such a run through two accessors,
// block(i) and mask(i), and on the items' popcount prefix, prefix(i) = set bits of the items in front of item i (of the
// whole sorted list: only differences are used).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SASSY_AMP_HD __host__ __device__ __forceinline__
#else
#define SASSY_AMP_HD inline
#endif

namespace sassy_hip {

constexpr uint64_t kAmpTileBytes = 4096;  // = kHamTileBlocks * 64: the text a wavefront of the scan owns

SASSY_AMP_HD uint32_t amp_popc(uint64_t x) {
  uint32_t c = 0;
  for (; x; x &= x - 1) ++c;
  return c;
}

// The partner window of a left hit at s: the partner starts p with max(min_len, a, b) <= p + b_partner - s <= max_len, a and b
// the pair's primer lengths (both sites lie inside the product), b_partner one of them.  false: the window is empty.
SASSY_AMP_HD bool amp_window(uint64_t s, uint64_t min_len, uint64_t max_len, uint32_t a, uint32_t b, uint32_t b_partner, uint64_t* lo,
                             uint64_t* hi) {
  uint64_t shortest = min_len;
  if (shortest < a) shortest = a;
  if (shortest < b) shortest = b;
  if (shortest > max_len) return false;
  *lo = s + shortest - b_partner;  // (shortest >= b_partner)
  *hi = s + max_len - b_partner;
  return true;
}

// the first i in [i0, i1) with block(i) >= b, i1 if there is none
template <typename Block>
SASSY_AMP_HD uint32_t amp_lower_bound(const Block& block, uint32_t i0, uint32_t i1, uint64_t b) {
  while (i0 < i1) {
    const uint32_t mid = i0 + (i1 - i0) / 2;
    if (block(mid) < b) i0 = mid + 1;
    else i1 = mid;
  }
  return i0;
}

// the starts of one item that lie in [lo, hi]
SASSY_AMP_HD uint64_t amp_clip(uint64_t block, uint64_t mask, uint64_t lo, uint64_t hi) {
  const uint64_t s0 = block * 64;
  if (lo > hi || s0 + 63 < lo || s0 > hi) return 0;
  if (lo > s0) mask &= ~(uint64_t)0 << (lo - s0);
  if (hi - s0 < 63) mask &= ((uint64_t)2 << (hi - s0)) - 1;
  return mask;
}

// The items of the run [i0, i1) that can hold a start of [lo, hi]: [*first, *last), possibly empty.
template <typename Block>
SASSY_AMP_HD void amp_span(const Block& block, uint32_t i0, uint32_t i1, uint64_t lo, uint64_t hi, uint32_t* first, uint32_t* last) {
  *first = *last = i0;
  if (lo > hi) return;
  *first = amp_lower_bound(block, i0, i1, lo / 64);
  *last = amp_lower_bound(block, *first, i1, hi / 64 + 1);
}

// How many starts of the run [i0, i1) lie in [lo, hi]: a partial first and last mask, whole masks in between -- those through
// the prefix, so absent blocks cost nothing.
template <typename Block, typename Mask, typename Prefix>
SASSY_AMP_HD uint64_t amp_count(const Block& block, const Mask& mask, const Prefix& prefix, uint32_t i0, uint32_t i1, uint64_t lo, uint64_t hi) {
  uint32_t first, last;
  amp_span(block, i0, i1, lo, hi, &first, &last);
  if (first >= last) return 0;
  uint64_t c = amp_popc(amp_clip(block(first), mask(first), lo, hi));
  if (last - first == 1) return c;
  c += amp_popc(amp_clip(block(last - 1), mask(last - 1), lo, hi));
  return c + (uint64_t)(prefix(last - 1) - prefix(first + 1));
}

// The j-th (from 0, ascending) start of the run [i0, i1) in [lo, hi]; false: there are j or fewer.
template <typename Block, typename Mask, typename Prefix>
SASSY_AMP_HD bool amp_select(const Block& block, const Mask& mask, const Prefix& prefix, uint32_t i0, uint32_t i1, uint64_t lo, uint64_t hi,
                             uint64_t j, uint64_t* start) {
  uint32_t first, last;
  amp_span(block, i0, i1, lo, hi, &first, &last);
  if (first >= last) return false;
  uint64_t m = amp_clip(block(first), mask(first), lo, hi);
  uint32_t at = first;
  const uint64_t c0 = amp_popc(m);
  if (j >= c0) {
    if (last - first == 1) return false;
    j -= c0;
    const uint64_t whole = (uint64_t)(prefix(last - 1) - prefix(first + 1));
    if (j < whole) {  // the last item of (first, last - 1) whose prefix, counted from first + 1, is <= j
      const uint64_t base = prefix(first + 1);
      uint32_t a = first + 1, b = last - 1;
      while (b - a > 1) {
        const uint32_t mid = a + (b - a) / 2;
        if ((uint64_t)(prefix(mid) - base) <= j) a = mid;
        else b = mid;
      }
      at = a;
      j -= (uint64_t)(prefix(a) - base);
      m = mask(a);
    } else {
      j -= whole;
      at = last - 1;
      m = amp_clip(block(at), mask(at), lo, hi);
      if (j >= amp_popc(m)) return false;
    }
  }
  for (; j; --j) m &= m - 1;
  uint32_t bit = 0;
  while (!((m >> bit) & 1u)) ++bit;
  *start = block(at) * 64 + bit;
  return true;
}

// Which range of tiles owns a left hit.  A range [t0, t1) of the scan holds every partner of a left hit at s when
// s + max_len <= t1 * 4096 (a partner starts in front of its product's end), or when the range is the text's last.  The
// ranges of a call overlap, so a range owns from `own_from` on -- the first start the range before it did not own, at or
// behind its own first byte -- and no start is owned twice.
SASSY_AMP_HD bool amp_owns(uint64_t s, uint64_t own_from, uint64_t t1, bool last, uint64_t max_len) {
  return s >= own_from && (last || s + max_len <= t1 * kAmpTileBytes);
}
// the first start that a range [.., t1) which is not the last does not own (own_from: its own)
SASSY_AMP_HD uint64_t amp_next_from(uint64_t own_from, uint64_t t1, uint64_t max_len) {
  const uint64_t end = t1 * kAmpTileBytes;
  const uint64_t next = end >= max_len ? end - max_len + 1 : 0;
  return next > own_from ? next : own_from;
}
// the fewest tiles of a range that is not the last and still moves the next range's first tile on: more than
// max_len / 4096 + 1
SASSY_AMP_HD uint64_t amp_min_span(uint64_t max_len) { return max_len / kAmpTileBytes + 2; }

}  // namespace sassy_hip
