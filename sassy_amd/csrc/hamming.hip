// hamming.hip -- sassy_hip_search_hamming: every start with at most k mismatches (substitutions only), counted on the device.
//
// No DP state: a block's answer depends on the text under it and on the W = ceil((m - 1) / 64) blocks to its right, so any
// split of the text is exact -- no seams, no warm-up, no report rule.  Two kernels:
//   ham_scan_kernel  a wavefront owns a tile of 64 consecutive blocks, a lane one block (64 starts).  The tile is staged
//                    with coalesced loads, every lane builds its block's slot masks once (profile_masks.h) and puts them
//                    into LDS as [slot][block] next to the masks of the tile's W halo blocks; then, per pattern of the
//                    launch, a row is two LDS words, a funnel shift and a bit-sliced add (hamming_step.h).  A non-zero hit
//                    mask leaves as one 16-byte item (pattern | strand, block, mask), one atomic per wavefront.
//   ham_emit_kernel  the items sorted by (pattern | strand, block) and their popcount prefix give every hit its record
//                    index: a lane per hit reads the m window bytes once for cost and cigar.
// sassy_hip_search_hamming_many / sassy_hip_hamming_best_pattern: a batch of texts in one buffer, each from a multiple of 64
// bytes on.  The scan kernel's MANY instantiations mask the starts by rem[block], the bytes left in the block's own text
// (ham_rem_kernel builds it on the device); the emit kernel finds a hit's text in the start table.  Best pattern: no items --
// the block's minimum (ham_min_cost) goes into one 64-bit cell per text.
// sassy_hip_hamming_counts / _counts_many: no items either -- the COUNT instantiations fold a wavefront's hits per cost
// (HamCounter::eq) into a table of 64-bit counters, one atomic per wavefront, pattern and present cost.
#include "host_internal.h"
#include "profile_masks.h"
#include "hamming_step.h"

namespace sassy_hip {
namespace {

static_assert(kHamMaxHalo == (kHamMaxRows - 1 + 63) / 64, "halo of the longest pattern");
static_assert((uint32_t)PROFILE_DNA == kHamDna && (uint32_t)PROFILE_IUPAC == kHamIupac && (uint32_t)PROFILE_ASCII_CI == kHamAsciiCi,
              "hamming_step.h names the profiles by value");

constexpr uint32_t kHamStageBytes = kHamTileBlocks * 64;  // a tile's text
constexpr uint32_t kHamLdsBudget = 160 * 1024;
// (HamItem, the pattern table's layout -- kHamTabWords, kHamNoFilter -- and HamPattern: host_internal.h)

struct HamParams {
  const uint8_t* text;
  uint64_t n;          // bytes
  uint64_t n_blocks;   // ceil(n / 64): blocks that may be loaded
  uint64_t tile0;      // this launch's tiles [tile0, tile0 + n_tiles)
  uint64_t n_tiles;
  uint32_t k, n_pat;
  uint32_t halo;       // halo blocks of the launch's longest pattern
  uint32_t nb;         // = 64 + halo: blocks per slot row in LDS
  uint32_t n_filter;   // some pattern of the launch has an N threshold
  uint32_t item_cap;
  const uint32_t* tab;
  const uint32_t* rows;
  HamItem* items;
  uint32_t* item_count;  // keeps counting past item_cap
};

// The batch of texts a MANY launch scans (all device pointers); unused by the single-text instantiations.
struct HamMany {
  const uint32_t* rem;          // per block: bytes from its first byte to its text's end, saturated
  const uint64_t* starts;       // per text: its first byte in the buffer
  uint32_t n_texts;
  unsigned long long* cells;    // != nullptr: best pattern -- per text cost:8 | 2 pattern_idx + strand:24 | start:32, all ones = none
};

// The table a COUNT launch adds into (hamming_counts); unused by the other instantiations.
struct HamCounts {
  unsigned long long* bins;  // (copy_mask + 1) copies of n_bins counters: bin (2 pattern_idx + strand) * stride + cost
  uint32_t n_bins;
  uint32_t stride;           // k + 1 of the call (the launch's k may be smaller: k >= m is cut to the longest pattern)
  uint32_t copy_mask;        // copies - 1, copies a power of two: a workgroup adds into copy blockIdx.x & copy_mask
};

// LDS of one wavefront: the staged tile, then (slots + 1) rows of nb masks -- the last row is the N mask --, whole 16 bytes
__host__ __device__ constexpr uint32_t ham_lds_per_wave(uint32_t slots, uint32_t nb) {
  return (kHamStageBytes + (slots + 1) * nb * 8u + 15u) & ~15u;
}

typedef const uint32_t __attribute__((address_space(4)))* ham_u32_ptr;  // scalar reads of wave-uniform tables

__device__ __forceinline__ uint2 n_mask(const uint32_t (&x)[16]) {  // bit i: text byte i is 'N' / 'n'
  uint32_t v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t d = (x[i] | 0x20202020u) ^ 0x6E6E6E6Eu;  // zero bytes are N
    const uint32_t nz = ((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d;
    v[i] = __builtin_amdgcn_udot4((~nz >> 7) & 0x01010101u, 0x08040201u, 0u, false);
  }
  uint2 r = make_uint2(0u, 0u);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    r.x |= v[i] << (4 * i);
    r.y |= v[8 + i] << (4 * i);
  }
  return r;
}

__device__ __forceinline__ uint32_t ham_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t ham_wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t ham_wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
  return v;
}

template <int PROFILE, int NS, int P, bool MANY, bool COUNT>
__global__ __launch_bounds__(256) void ham_scan_kernel(const HamParams H, const ScanParams SP, const HamMany M, const HamCounts C) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ham_lds[];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, wpg = blockDim.x >> 6;
  const uint64_t t_rel = (uint64_t)blockIdx.x * wpg + wave;
  if (t_rel >= H.n_tiles) return;  // (waves work alone: no workgroup barrier anywhere)
  const uint64_t tile = H.tile0 + t_rel;
  const uint32_t per_wave = ham_lds_per_wave((uint32_t)NS, H.nb);
  unsigned char* stage = ham_lds + (size_t)wave * per_wave;
  unsigned char* masks = stage + kHamStageBytes;  // [slot][block], slot NS = the N mask
  const uint64_t block = tile * kHamTileBlocks + lane;

  // the tile's text: 16-byte slot q (owner lane q >> 2, chunk q & 3) of the tile, loaded 1 KiB per instruction, kept at
  // 4 owner + (chunk ^ ((owner >> 2) & 3)) so that the owners' 16-byte reads spread over the banks
  const uint64_t tile_byte = tile * (uint64_t)kHamStageBytes, loadable = H.n_blocks * 64;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t q = i * 64u + lane, owner = q >> 2, chunk = q & 3u;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (tile_byte + (uint64_t)q * 16 < loadable) v = *reinterpret_cast<const uint4*>(H.text + tile_byte + (uint64_t)q * 16);
    *reinterpret_cast<uint4*>(stage + (4u * owner + (chunk ^ ((owner >> 2) & 3u))) * 16u) = v;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // pass 0: every lane its own block; pass 1: lanes < halo the tile's halo blocks (never loaded behind the text's end)
#pragma unroll 1
  for (uint32_t pass = 0; pass < 2; ++pass) {
    if (pass == 1 && H.halo == 0) break;
    const bool on = pass == 0 || lane < H.halo;
    uint32_t x[16];
    if (pass == 0) {
#pragma unroll
      for (uint32_t c = 0; c < 4; ++c) {
        const uint4 v = *reinterpret_cast<const uint4*>(stage + (4u * lane + (c ^ ((lane >> 2) & 3u))) * 16u);
        x[4 * c] = v.x; x[4 * c + 1] = v.y; x[4 * c + 2] = v.z; x[4 * c + 3] = v.w;
      }
    } else {
      const uint64_t hb = (tile + 1) * kHamTileBlocks + lane;
      const bool load = on && hb < H.n_blocks;
#pragma unroll
      for (uint32_t c = 0; c < 4; ++c) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (load) v = *reinterpret_cast<const uint4*>(H.text + hb * 64 + c * 16u);
        x[4 * c] = v.x; x[4 * c + 1] = v.y; x[4 * c + 2] = v.z; x[4 * c + 3] = v.w;
      }
    }
    const uint64_t my_block = pass == 0 ? block : (tile + 1) * kHamTileBlocks + lane;
    const bool inside = my_block < H.n_blocks;  // a block behind the text matches nothing
    uint2 msk[NS];
    build_masks<PROFILE, NS>(x, SP, msk);
    const uint32_t col = pass * kHamTileBlocks + lane;
    if (on) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
        *reinterpret_cast<uint2*>(masks + ((size_t)s * H.nb + col) * 8u) = inside ? msk[s] : make_uint2(0u, 0u);
      if (H.n_filter) *reinterpret_cast<uint2*>(masks + ((size_t)NS * H.nb + col) * 8u) = inside ? n_mask(x) : make_uint2(0u, 0u);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  const ham_u32_ptr tab = (ham_u32_ptr)H.tab;
  const ham_u32_ptr rows = (ham_u32_ptr)H.rows;
  const uint32_t nb = H.nb;
  auto fetch = [&](uint32_t slot, uint32_t q) {
    return *reinterpret_cast<const uint64_t*>(masks + ((size_t)slot * nb + lane + q) * 8u);
  };
  auto all_over = [](uint64_t over) { return __all(over == ~(uint64_t)0) != 0; };
  uint32_t rem = 0;  // (MANY) what is left of this block's own text; a block behind the buffer has none
  if constexpr (MANY) rem = block < H.n_blocks ? M.rem[block] : 0u;
  for (uint32_t p = 0; p < H.n_pat; ++p) {
    const uint32_t m = tab[kHamTabWords * p], roff = tab[kHamTabWords * p + 1], nmax = tab[kHamTabWords * p + 3];
    auto row_word = [&](uint32_t w) { return rows[roff + w]; };
    HamCounter<P> cnt;
    ham_count<P, true>(fetch, row_word, m, all_over, cnt);
    uint64_t hit = cnt.le(H.k) & (MANY ? ham_valid_mask_rem(rem, m) : ham_valid_mask(block, H.n, m));
    // the N filter, before a hit takes list space -- and only where some block of the tile holds a hit
    if (nmax != kHamNoFilter && __any(hit != 0)) {
      auto n_word = [](uint32_t) { return (uint32_t)NS * 0x01010101u; };
      hit &= ham_hit_mask<kHamNPlanes, false>(fetch, n_word, m, nmax, all_over);
    }
    if constexpr (COUNT) {
      // hamming_counts: the hits of the wavefront per cost.  `hit` is what search_hamming would list (position mask and N
      // filter are behind it) and every start in it has an exact count <= H.k <= C.stride - 1 (HamCounter::eq).  Two wave
      // reductions bound the costs that are present; per cost one wave sum and one add without a return value by one lane.
      if (__any(hit != 0)) {
        uint64_t at;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)ham_wave_min(ham_min_cost<P>(cnt, hit, &at)));
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)ham_wave_max(ham_max_cost<P>(cnt, hit)));
        unsigned long long* row = C.bins + (size_t)(blockIdx.x & C.copy_mask) * C.n_bins +
                                  (size_t)(2u * tab[kHamTabWords * p + 4] + tab[kHamTabWords * p + 5]) * C.stride;
        for (uint32_t c = lo; c <= hi; ++c) {
          const uint32_t sum = ham_wave_sum((uint32_t)__builtin_popcountll(cnt.eq(c) & hit));
          if (sum != 0 && lane == 0) (void)__hip_atomic_fetch_add(row + c, (unsigned long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      continue;
    }
    if constexpr (MANY) {
      if (M.cells) {  // best pattern: the block's minimum into its text's cell, the key's order is the tie order
        if (hit != 0) {
          uint64_t at;
          const uint32_t cost = ham_min_cost<P>(cnt, hit, &at);
          const uint64_t s = block * 64 + (uint32_t)__builtin_ctzll(at);
          const uint32_t t = ham_text_of([&](uint32_t i) { return M.starts[i]; }, M.n_texts, s);
          const uint64_t who = 2ull * tab[kHamTabWords * p + 4] + tab[kHamTabWords * p + 5];
          const unsigned long long key = ((unsigned long long)cost << 56) | (who << 32) | (uint32_t)(s - M.starts[t]);
          if (M.cells[t] > key) atomicMin(M.cells + t, key);
        }
        continue;
      }
    }
    const bool has = hit != 0;
    const uint64_t bal = __ballot(has);
    if (bal != 0) {
      const uint32_t first = (uint32_t)__builtin_ctzll(bal);
      uint32_t base = 0;
      if (lane == first) base = atomicAdd(H.item_count, (uint32_t)__builtin_popcountll(bal));
      base = __shfl(base, (int)first);
      const uint32_t at = base + (uint32_t)__builtin_popcountll(bal & (((uint64_t)1 << lane) - 1));
      if (has && at < H.item_cap) H.items[at] = HamItem{((uint64_t)p << 32) | (uint32_t)block, hit};
    }
  }
}

// rem[b] for every block of a laid-out batch, from the (start, len) table: a thread per block
__global__ __launch_bounds__(256) void ham_rem_kernel(const uint64_t* __restrict__ starts, const uint64_t* __restrict__ lens, uint32_t n_texts,
                                                      uint64_t n_blocks, uint32_t* __restrict__ rem) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks) return;
  const uint32_t t = ham_text_of([&](uint32_t i) { return starts[i]; }, n_texts, b * 64);
  rem[b] = ham_rem(b, starts[t], lens[t]);
}

struct EmitParams {
  const uint8_t* text;
  const HamItem* items;      // sorted
  const uint32_t* prefix;    // prefix[i] = hits of the items in front of item i
  uint32_t n_items;
  uint32_t first, count;     // this launch: hits [first, first + count) of the range
  const uint32_t* tab;
  const uint8_t* pats;       // the patterns as scanned
  uint32_t profile;
  uint32_t str_stride;       // 0: without trace
  MatchOut* out;             // count records
  char* strs;                // count * str_stride bytes
  const uint64_t* starts;    // != nullptr: the text is a batch of n_texts texts, the records are relative to their text
  uint32_t n_texts;
  uint64_t text0;            // index of the batch's first text in the call
};

__global__ __launch_bounds__(256) void ham_emit_kernel(const EmitParams E) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= E.count) return;
  const uint32_t r = E.first + t;
  uint32_t lo = 0, hi = E.n_items;  // the last item whose prefix is <= r
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (E.prefix[mid] <= r) lo = mid;
    else hi = mid;
  }
  const HamItem it = E.items[lo];
  uint64_t mask = it.mask;
  for (uint32_t skip = r - E.prefix[lo]; skip; --skip) mask &= mask - 1;
  const uint64_t s = (it.key & 0xFFFFFFFFull) * 64 + (uint32_t)__builtin_ctzll(mask);
  const uint32_t* row = E.tab + kHamTabWords * (uint32_t)(it.key >> 32);
  const uint32_t m = row[0], strand = row[5];
  const uint8_t* win = E.text + s;
  uint32_t cost, n_count, cigar_len;
  ham_emit_hit(E.profile, E.pats + row[2], m, [&](uint32_t i) { return (uint32_t)win[i]; }, strand != 0,
               E.str_stride ? E.strs + (size_t)t * E.str_stride : nullptr, &cost, &n_count, &cigar_len);
  MatchOut o{};
  o.pattern_idx = row[4];
  uint64_t rel = s;
  o.text_idx = 0;
  if (E.starts) {
    const uint32_t ti = ham_text_of([&](uint32_t i) { return E.starts[i]; }, E.n_texts, s);
    rel = s - E.starts[ti];
    o.text_idx = E.text0 + ti;
  }
  o.text_start = rel;
  o.text_end = rel + m;
  o.pattern_start = 0;
  o.pattern_end = m;
  o.cost = (int32_t)cost;
  o.strand = (uint8_t)strand;
  o.cigar_off = t * E.str_stride;
  o.cigar_len = cigar_len;
  E.out[t] = o;
}

template <int PROFILE, int NS, int P, bool MANY, bool COUNT>
hipError_t launch_scan_k(const HamParams& H, const ScanParams& SP, const HamMany& M, const HamCounts& C, uint32_t grid, uint32_t threads,
                         size_t smem, hipStream_t st) {
  static DeviceOnce attr_set;  // LDS beyond the 64 KiB default needs an explicit opt-in
  if (attr_set.need()) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ham_scan_kernel<PROFILE, NS, P, MANY, COUNT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHamLdsBudget);
    if (e != hipSuccess) return e;
    attr_set.done();
  }
  hipLaunchKernelGGL((ham_scan_kernel<PROFILE, NS, P, MANY, COUNT>), dim3(grid), dim3(threads), smem, st, H, SP, M, C);
  return hipGetLastError();
}

template <int PROFILE, int NS, bool MANY, bool COUNT>
hipError_t launch_scan_p(const HamParams& H, const ScanParams& SP, const HamMany& M, const HamCounts& C, uint32_t grid, uint32_t threads,
                         size_t smem, hipStream_t st) {
  switch (ham_planes(H.k)) {
    case 2: return launch_scan_k<PROFILE, NS, 2, MANY, COUNT>(H, SP, M, C, grid, threads, smem, st);
    case 4: return launch_scan_k<PROFILE, NS, 4, MANY, COUNT>(H, SP, M, C, grid, threads, smem, st);
    case 8: return launch_scan_k<PROFILE, NS, 8, MANY, COUNT>(H, SP, M, C, grid, threads, smem, st);
    default: return launch_scan_k<PROFILE, NS, 11, MANY, COUNT>(H, SP, M, C, grid, threads, smem, st);
  }
}

template <bool MANY, bool COUNT>
hipError_t launch_scan_m(Profile pr, uint32_t ns, const HamParams& H, const ScanParams& SP, const HamMany& M, const HamCounts& C, uint32_t grid,
                         uint32_t threads, size_t smem, hipStream_t st) {
  switch (pr) {
    case PROFILE_DNA: return launch_scan_p<(int)PROFILE_DNA, 4, MANY, COUNT>(H, SP, M, C, grid, threads, smem, st);
    case PROFILE_IUPAC: return launch_scan_p<(int)PROFILE_IUPAC, 16, MANY, COUNT>(H, SP, M, C, grid, threads, smem, st);
    case PROFILE_ASCII_CI:
      return ns <= 16 ? launch_scan_p<(int)PROFILE_ASCII_CI, 16, MANY, COUNT>(H, SP, M, C, grid, threads, smem, st)
                      : launch_scan_p<(int)PROFILE_ASCII_CI, 64, MANY, COUNT>(H, SP, M, C, grid, threads, smem, st);
    default:
      return ns <= 16 ? launch_scan_p<(int)PROFILE_ASCII, 16, MANY, COUNT>(H, SP, M, C, grid, threads, smem, st)
                      : launch_scan_p<(int)PROFILE_ASCII, 64, MANY, COUNT>(H, SP, M, C, grid, threads, smem, st);
  }
}

// many == nullptr: one text; counts != nullptr: the COUNT instantiations
hipError_t launch_scan(Profile pr, uint32_t ns, const HamParams& H, const ScanParams& SP, const HamMany* many, const HamCounts* counts,
                       uint32_t grid, uint32_t threads, size_t smem, hipStream_t st) {
  if (counts)
    return many ? launch_scan_m<true, true>(pr, ns, H, SP, *many, *counts, grid, threads, smem, st)
                : launch_scan_m<false, true>(pr, ns, H, SP, HamMany{}, *counts, grid, threads, smem, st);
  return many ? launch_scan_m<true, false>(pr, ns, H, SP, *many, HamCounts{}, grid, threads, smem, st)
              : launch_scan_m<false, false>(pr, ns, H, SP, HamMany{}, HamCounts{}, grid, threads, smem, st);
}

uint32_t slot_byte(Profile pr, uint8_t c) {  // what a pattern byte's slot is keyed by
  if (pr == PROFILE_DNA) return (c >> 1) & 3u;
  if (pr == PROFILE_IUPAC) return iupac_code(c) & 0x0Fu;
  return pr == PROFILE_ASCII_CI ? fold_ascii(c) : c;
}

}  // namespace

// A laid-out batch of texts on the device (hamming_many_on_device): d_text is the whole buffer, n its size.
struct HamTexts {
  HamMany dev;
  uint64_t text0;    // index of the batch's first text in the call
  uint64_t longest;  // the batch's longest text
};

// The tables of a launch group (HamRange, host_internal.h): tab, rows and pats built and uploaded, the launch's shape, the
// item list's sizes.
static int ham_prepare(sassy_SearcherType* S, HamRange& G) {
  const Profile pr = S->profile;
  ScanLane& L = S->lanes[0];
  const uint32_t np = G.np, ns = G.ns;
  const long items_sw = S->sw.hamming_items;
  std::vector<uint32_t>& tab = G.tab;
  tab.assign((size_t)np * kHamTabWords, 0u);
  std::vector<uint32_t> rows;
  std::vector<uint8_t> pats;
  uint32_t longest = 0;
  bool n_filter = false;
  for (uint32_t p = 0; p < np; ++p) {
    const HamPattern& hp = G.pats[p];
    const uint32_t m = (uint32_t)hp.bytes.size();
    longest = std::max(longest, m);
    const uint32_t nmax = hp.nmax;
    uint32_t* row = &tab[(size_t)p * kHamTabWords];
    row[0] = m; row[1] = (uint32_t)rows.size(); row[2] = (uint32_t)pats.size(); row[3] = nmax; row[4] = hp.idx; row[5] = hp.strand;
    n_filter = n_filter || nmax != kHamNoFilter;
    rows.resize(rows.size() + (m + 3) / 4, 0u);
    for (uint32_t j = 0; j < m; ++j) rows[row[1] + (j >> 2)] |= (uint32_t)G.slot_of[slot_byte(pr, hp.bytes[j])] << (8 * (j & 3));
    pats.insert(pats.end(), hp.bytes.begin(), hp.bytes.end());
  }
  G.longest = longest;
  G.n_filter = n_filter;
  G.halo = ham_halo_blocks(longest);
  G.nb = kHamTileBlocks + G.halo;
  const uint32_t ns_t = pr == PROFILE_DNA ? 4u : (pr == PROFILE_IUPAC || ns <= 16) ? 16u : 64u;
  const uint32_t per_wave = ham_lds_per_wave(ns_t, G.nb);
  G.wpg = std::min<uint32_t>(4, kHamLdsBudget / per_wave);
  G.smem = (size_t)G.wpg * per_wave;

  if (int rc = S->d_ham_tab.reserve(tab.size() + rows.size() + (pats.size() + 3) / 4 + 16)) return rc;
  G.d_tab = S->d_ham_tab.p;
  G.d_rows = G.d_tab + tab.size();
  G.d_pats = reinterpret_cast<uint8_t*>(G.d_rows + rows.size());
  if (int rc = S->d_ham_count.reserve(16)) return rc;
  L.h_up_used = 0;
  if (int rc = L.upload(G.d_tab, tab.data(), tab.size() * 4)) return rc;
  if (int rc = L.upload(G.d_rows, rows.data(), rows.size() * 4)) return rc;
  if (int rc = L.upload(G.d_pats, pats.data(), pats.size())) return rc;

  const uint64_t min_cap = (uint64_t)np * kHamTileBlocks;  // one tile always fits
  G.item_cap = std::max<uint64_t>(items_sw > 0 ? (uint64_t)items_sw : (1u << 16), min_cap);
  G.max_cap = items_sw > 0 ? G.item_cap : std::max<uint64_t>(min_cap, 1u << 22);
  G.span_max = std::max<uint64_t>(1, (0x7FFFFFFFull / kHamTileBlocks) / np);  // the counter cannot wrap
  G.ready = true;
  return 0;
}

// One range of a launch group's tiles: the scan, the counter, a list that overflows (a larger list, or a shorter range, and
// the launch again), the sort by (pattern | strand, block), the items on the host.
int ham_scan_range(sassy_SearcherType* S, HamRange& G) {
  if (!G.ready)
    if (int rc = ham_prepare(S, G)) return rc;
  const Profile pr = S->profile;
  hipStream_t st = S->stream;
  ScanLane& L = S->lanes[0];
  const bool timed = S->timing >= 1;
  const uint64_t n_blocks = (G.n + 63) / 64, n_tiles = (n_blocks + kHamTileBlocks - 1) / kHamTileBlocks;
  const uint32_t np = G.np, wpg = G.wpg;
  G.span = std::min(G.span, G.span_max);
  G.overflow = false;
  G.items.clear();
  uint32_t count = 0;
  for (;;) {
    uint64_t& span = G.span;
    uint64_t& item_cap = G.item_cap;
    const uint64_t max_cap = G.max_cap;
    span = std::min(span, n_tiles - G.tile0);
    if (int rc = S->d_ham_items.reserve(item_cap)) return rc;
    HamParams H{};
    H.text = G.d_text; H.n = G.n; H.n_blocks = n_blocks; H.tile0 = G.tile0; H.n_tiles = span;
    H.k = G.k; H.n_pat = np; H.halo = G.halo; H.nb = G.nb; H.n_filter = G.n_filter ? 1u : 0u; H.item_cap = (uint32_t)item_cap;
    H.tab = G.d_tab; H.rows = G.d_rows; H.items = reinterpret_cast<HamItem*>(S->d_ham_items.p); H.item_count = S->d_ham_count.p;
    HIP_TRY(hipMemsetAsync(S->d_ham_count.p, 0, 4, st));
    if (timed) HIP_TRY(hipEventRecord(L.ev_a, st));
    const uint32_t grid = (uint32_t)((span + wpg - 1) / wpg);
    HIP_TRY(launch_scan(pr, G.ns, H, G.SP, G.many ? &G.many->dev : nullptr, nullptr, grid, wpg * 64, G.smem, st));
    if (timed) HIP_TRY(hipEventRecord(L.ev_b, st));
    HIP_TRY(hipMemcpyAsync(&count, S->d_ham_count.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (timed) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, L.ev_a, L.ev_b) == hipSuccess) S->stats.scan_ms += ms;
    }
    S->stats.scan_launches += 1;
    S->stats.grid = grid;
    if (count <= item_cap) break;
    // nothing of this launch is used: a larger list, or a shorter range
    if (item_cap < max_cap && (uint64_t)count <= max_cap) item_cap = std::min<uint64_t>(max_cap, (uint64_t)count + count / 4);
    else if (item_cap < max_cap) item_cap = max_cap;
    if (count > item_cap) {
      if (span <= G.min_span) {  // (never with min_span == 1: one tile always fits)
        G.overflow = true;
        G.count = count;
        return 0;
      }
      span = std::max<uint64_t>(G.min_span, std::min<uint64_t>(span - 1, span * item_cap / count));
    }
  }
  G.count = count;
  S->stats.blocks += std::min<uint64_t>(G.span * kHamTileBlocks, n_blocks - G.tile0 * kHamTileBlocks);
  S->stats.hit_blocks += count;
  if (count) {
    // items by (pattern | strand, block)
    if (int rc = S->d_ham_sorted.reserve(count)) return rc;
    const size_t sb = sort_scratch_bytes(count);
    if (int rc = S->d_ham_sort.reserve(sb)) return rc;
    int key_bits = 33;
    while (key_bits < 64 && ((uint64_t)(np - 1) >> (key_bits - 32)) != 0) ++key_bits;
    HIP_TRY(launch_sort_candidates(S->d_ham_items.p, S->d_ham_sorted.p, count, S->d_ham_sort.p, S->d_ham_sort.cap, st, 0, key_bits));
    G.items.resize(count);
    HIP_TRY(hipMemcpyAsync(G.items.data(), S->d_ham_sorted.p, (size_t)count * sizeof(HamItem), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return 0;
}

// The search proper: refusals are the caller's; d_text is readable up to the next multiple of 64 bytes.  many != nullptr:
// d_text is a batch of texts; with many->dev.cells the launches reduce into the cells and R stays as it is.  counts != nullptr:
// the launches add into the table, nothing is listed and R is not touched (it may be nullptr).
static int hamming_on_device(sassy_SearcherType* S, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                             const uint8_t* d_text, uint64_t n, uint32_t k, bool without_trace, sassy_hip_Result* R,
                             const HamTexts* many = nullptr, const HamCounts* counts = nullptr) {
  const Profile pr = S->profile;
  hipStream_t st = S->stream;
  ScanLane& L = S->lanes[0];
  const uint64_t n_blocks = (n + 63) / 64, n_tiles = (n_blocks + kHamTileBlocks - 1) / kHamTileBlocks;
  if (n_blocks + kHamMaxHalo > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "text too long for the Hamming search (2^32 blocks)");
  S->stats.filtered = 7;
  S->stats.blocks_per_chunk = kHamTileBlocks;

  // the patterns as scanned, in the contract's order: pattern, then + before -
  std::vector<HamPattern> all;
  for (size_t i = 0; i < n_patterns; ++i) {
    const uint32_t m = (uint32_t)pattern_lens[i];
    uint32_t nmax = kHamNoFilter;
    if (!std::isnan(S->max_n_frac)) {
      const int64_t c = ham_n_max(m, S->max_n_frac);
      if (c < 0) continue;  // not even a span without N passes: the pattern has no hits
      if (c < (int64_t)m) nmax = (uint32_t)c;
    }
    if ((many ? many->longest : n) < m) continue;
    all.push_back(HamPattern{(uint32_t)i, 0, std::vector<uint8_t>(patterns[i], patterns[i] + m), nmax});
    if (S->rc) {
      HamPattern rc{(uint32_t)i, 1, {}, nmax};
      for (size_t j = m; j-- > 0;) rc.bytes.push_back(complement_char(pr, patterns[i][j]));
      all.push_back(std::move(rc));
    }
  }
  const long batch_sw = S->sw.hamming_batch, records_sw = S->sw.hamming_records;
  const size_t max_batch = batch_sw > 0 ? (size_t)batch_sw : 512;
  const bool timed = S->timing >= 1;

  size_t a0 = 0;
  while (a0 < all.size()) {
    // ---- a launch's patterns: as many as share the slots (Ascii: at most kMaxSlots distinct bytes) ----
    HamRange G;
    ham_slots_init(pr, G);
    uint32_t& ns = G.ns;
    int* slot_of = G.slot_of;
    ScanParams& SP = G.SP;
    size_t a1 = a0;
    while (a1 < all.size() && a1 - a0 < max_batch) {
      uint32_t add = 0;
      bool seen[256] = {};
      if (is_ascii(pr))
        for (uint8_t c : all[a1].bytes) {
          const uint32_t key = slot_byte(pr, c);
          if (slot_of[key] < 0 && !seen[key]) { seen[key] = true; ++add; }
        }
      if (ns + add > (uint32_t)kMaxSlots) break;  // (a pattern alone always fits: the caller checked)
      if (is_ascii(pr))
        for (uint8_t c : all[a1].bytes) {
          const uint32_t key = slot_byte(pr, c);
          if (slot_of[key] < 0) { slot_of[key] = (int)ns; SP.slot_val[ns++] = (uint8_t)key; }
        }
      ++a1;
    }
    SP.nslots = ns;
    SP.profile = (uint32_t)pr;
    const uint32_t np = (uint32_t)(a1 - a0);
    G.pats = &all[a0]; G.np = np;
    G.d_text = d_text; G.n = n; G.k = k; G.many = many;
    if (int rc = ham_prepare(S, G)) return rc;
    const uint32_t longest = G.longest, halo = G.halo, nb = G.nb, wpg = G.wpg;
    const bool n_filter = G.n_filter;
    const size_t smem = G.smem;
    uint32_t* d_tab = G.d_tab;
    uint32_t* d_rows = G.d_rows;
    uint8_t* d_pats = G.d_pats;

    // ---- the text in ranges of tiles: a range whose items overflow the list is cut down and launched again ----
    const uint64_t rec_cap = records_sw > 0 ? (uint64_t)records_sw : (1u << 20);
    const uint64_t span_max = G.span_max;
    if (counts || (many && many->dev.cells)) {  // counts, best pattern: nothing is listed, one launch takes every tile
      HamParams H{};
      H.text = d_text; H.n = n; H.n_blocks = n_blocks; H.tile0 = 0; H.n_tiles = n_tiles;
      H.k = k; H.n_pat = np; H.halo = halo; H.nb = nb; H.n_filter = n_filter ? 1u : 0u; H.item_cap = 0;
      H.tab = d_tab; H.rows = d_rows; H.items = nullptr; H.item_count = nullptr;
      if (timed) HIP_TRY(hipEventRecord(L.ev_a, st));
      const uint32_t grid = (uint32_t)((n_tiles + wpg - 1) / wpg);
      HIP_TRY(launch_scan(pr, ns, H, SP, many ? &many->dev : nullptr, counts, grid, wpg * 64, smem, st));
      if (timed) HIP_TRY(hipEventRecord(L.ev_b, st));
      HIP_TRY(hipStreamSynchronize(st));  // (the next group reuses the pinned upload area)
      if (timed) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, L.ev_a, L.ev_b) == hipSuccess) S->stats.scan_ms += ms;
      }
      S->stats.scan_launches += 1;
      S->stats.grid = grid;
      S->stats.blocks += n_blocks;
      S->stats.text_bytes += n;
      a0 = a1;
      continue;
    }
    uint64_t tile0 = 0;
    G.span = std::min(n_tiles, span_max);
    size_t first_row = R->matches.size();
    uint32_t ranges = 0;
    while (tile0 < n_tiles) {
      G.tile0 = tile0;
      if (int rc = ham_scan_range(S, G)) return rc;
      const uint32_t count = G.count;
      const std::vector<HamItem>& items = G.items;
      ++ranges;
      if (count) {
        // the items' popcount prefix
        std::vector<uint32_t> prefix(count);
        uint64_t hits = 0;
        for (uint32_t i = 0; i < count; ++i) {
          prefix[i] = (uint32_t)hits;
          hits += (uint64_t)__builtin_popcountll(items[i].mask);
        }
        if (hits > 0xFFFFFFFFull || R->matches.size() + hits > 0xFFFFFFFFull)
          return fail(SASSY_HIP_ENOMEM, "Hamming search: more than 2^32 records (" + std::to_string(R->matches.size() + hits) + ")");
        if (int rc = S->d_ham_prefix.reserve(count)) return rc;
        HIP_TRY(hipMemcpyAsync(S->d_ham_prefix.p, prefix.data(), (size_t)count * 4, hipMemcpyHostToDevice, st));
        // records in batches of the record block
        const uint32_t stride = without_trace ? 0u : 2u * longest + 8u;
        const uint64_t batch = std::min<uint64_t>(hits, rec_cap);
        if (int rc = L.d_trace.reserve(batch)) return rc;
        if (stride)
          if (int rc = L.d_str.reserve(batch * stride)) return rc;
        std::vector<MatchOut> rows_h;
        std::vector<char> strs_h;
        for (uint64_t r0 = 0; r0 < hits; r0 += batch) {
          const uint32_t cnt = (uint32_t)std::min<uint64_t>(batch, hits - r0);
          EmitParams E{};
          E.text = d_text; E.items = reinterpret_cast<const HamItem*>(S->d_ham_sorted.p); E.prefix = S->d_ham_prefix.p; E.n_items = count;
          E.first = (uint32_t)r0; E.count = cnt; E.tab = d_tab; E.pats = d_pats; E.profile = (uint32_t)pr; E.str_stride = stride;
          E.out = L.d_trace.p; E.strs = reinterpret_cast<char*>(L.d_str.p);
          if (many) { E.starts = many->dev.starts; E.n_texts = many->dev.n_texts; E.text0 = many->text0; }
          hipLaunchKernelGGL(ham_emit_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, E);
          HIP_TRY(hipGetLastError());
          rows_h.resize(cnt);
          if (int rc = L.download(rows_h.data(), L.d_trace.p, (size_t)cnt * sizeof(MatchOut))) return rc;
          if (stride) {
            strs_h.resize((size_t)cnt * stride);
            if (int rc = L.download(strs_h.data(), L.d_str.p, strs_h.size())) return rc;
          }
          HIP_TRY(hipStreamSynchronize(st));
          for (uint32_t i = 0; i < cnt; ++i) {
            sassy_hip_Match mo;
            memcpy(&mo, &rows_h[i], sizeof(mo));
            if (R->pool.size() + mo.cigar_len + 1 > 0xFFFFFFFFull)
              return fail(SASSY_HIP_ENOMEM, "Hamming search: more than 4 GiB of cigar text");
            const uint32_t off = (uint32_t)R->pool.size();
            if (stride) R->pool.append(strs_h.data() + (size_t)i * stride, mo.cigar_len);
            R->pool.push_back('\0');
            mo.cigar_off = off;
            R->matches.push_back(mo);
          }
        }
        S->stats.candidates += hits;
      }
      tile0 += G.span;
      G.span = std::min(n_tiles, span_max);  // the next range tries everything that is left
    }
    // several ranges: each came sorted by (pattern, strand, start); the ranges ascend, so a stable sort restores the order
    if (ranges > 1)
      std::stable_sort(R->matches.begin() + (long)first_row, R->matches.end(), [](const sassy_hip_Match& a, const sassy_hip_Match& b) {
        return a.pattern_idx != b.pattern_idx ? a.pattern_idx < b.pattern_idx : a.strand < b.strand;
      });
    S->stats.text_bytes += n;
    a0 = a1;
  }
  S->stats.chunks = n_tiles;
  return 0;
}

// A batch call: the texts in batches of at most `hamming_many_batch` bytes laid out, each text from a multiple of 64 bytes on
// (an empty text takes no block).  Records into R in the contract's order, or -- cells != nullptr -- per text of the call
// its best-pattern cell (all ones: no hit), nothing into R; or -- counts != nullptr -- every batch adds into the one table.
static int hamming_many_on_device(sassy_SearcherType* S, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                  const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, uint32_t k, bool without_trace,
                                  sassy_hip_Result* R, unsigned long long* cells, const HamCounts* counts = nullptr) {
  hipStream_t st = S->stream;
  const uint64_t batch_cap = S->sw.hamming_many_batch > 0 ? (uint64_t)S->sw.hamming_many_batch : (1ull << 30);
  HostTexts ht;
  uint64_t all_tiles = 0;
  size_t t0 = 0;
  while (t0 < n_texts) {
    size_t t1 = t0;
    uint64_t total = 0, longest = 0;
    ht.start.clear(); ht.len.clear();
    while (t1 < n_texts) {
      const uint64_t slot = ((uint64_t)text_lens[t1] + 63) / 64 * 64;
      if (t1 > t0 && total + slot > batch_cap) break;
      ht.start.push_back(total);
      ht.len.push_back(text_lens[t1]);
      longest = std::max<uint64_t>(longest, text_lens[t1]);
      total += slot;
      ++t1;
    }
    const size_t nt = t1 - t0;
    if (total == 0 || nt > 0xFFFFFFFFull) {  // (only empty texts: no hits)
      if (nt > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "Hamming search: more than 2^32 texts in one batch");
      t0 = t1;
      continue;
    }
    if (int rc = S->reserve_stage(total + 64)) return rc;
    if (int rc = S->d_text.reserve(total + 64)) return rc;
    if (int rc = layout_and_upload(S->h_stage, S->d_text.p, texts + t0, text_lens + t0, ht.start.data(), nt, total, (uint8_t)0, st)) return rc;
    const uint64_t n_blocks = total / 64;
    if (int rc = S->d_ham_texts.reserve(2 * nt)) return rc;
    if (int rc = S->d_ham_rem.reserve(n_blocks)) return rc;
    HIP_TRY(hipMemcpyAsync(S->d_ham_texts.p, ht.start.data(), nt * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S->d_ham_texts.p + nt, ht.len.data(), nt * 8, hipMemcpyHostToDevice, st));
    if (n_blocks + 255 > 0xFFFFFFFFull * 256ull) return fail(SASSY_HIP_EUNSUPPORTED, "text batch too long for the Hamming search");
    hipLaunchKernelGGL(ham_rem_kernel, dim3((uint32_t)((n_blocks + 255) / 256)), dim3(256), 0, st, S->d_ham_texts.p, S->d_ham_texts.p + nt,
                       (uint32_t)nt, n_blocks, S->d_ham_rem.p);
    HIP_TRY(hipGetLastError());
    HamTexts B{};
    B.dev.rem = S->d_ham_rem.p; B.dev.starts = S->d_ham_texts.p; B.dev.n_texts = (uint32_t)nt; B.dev.cells = nullptr;
    B.text0 = t0; B.longest = longest;
    if (cells) {
      if (int rc = S->d_ham_cells.reserve(nt)) return rc;
      HIP_TRY(hipMemsetAsync(S->d_ham_cells.p, 0xFF, nt * 8, st));
      B.dev.cells = S->d_ham_cells.p;
    }
    if (int rc = hamming_on_device(S, patterns, pattern_lens, n_patterns, S->d_text.p, total, k, without_trace, R, &B, counts)) return rc;
    if (cells) HIP_TRY(hipMemcpyAsync(cells + t0, S->d_ham_cells.p, nt * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the tables of the next batch overwrite this one's)
    all_tiles += S->stats.chunks;
    t0 = t1;
  }
  S->stats.chunks = all_tiles;
  S->stats.filtered = 7;
  S->stats.blocks_per_chunk = kHamTileBlocks;
  // batches, pattern groups and ranges each came in the contract's order, and all of them ascend in text order: a stable
  // sort on (pattern, strand) restores it for the call
  auto by_pattern = [](const sassy_hip_Match& a, const sassy_hip_Match& b) {
    return a.pattern_idx != b.pattern_idx ? a.pattern_idx < b.pattern_idx : a.strand < b.strand;
  };
  if (R && !std::is_sorted(R->matches.begin(), R->matches.end(), by_pattern)) std::stable_sort(R->matches.begin(), R->matches.end(), by_pattern);
  return 0;
}

// What every Hamming entry point refuses, before any device work; `who` names the entry point.
static int hamming_refusals(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns, size_t k,
                            const char* who) {
  if (!std::isnan(s->alpha) || s->max_overhang >= 0)
    return fail(SASSY_HIP_EUNSUPPORTED, "the Hamming search does not take overhang (alpha): a hit spans the whole pattern");
  if (s->only_best) return fail(SASSY_HIP_EUNSUPPORTED, "the Hamming search reports every hit: only_best_match is not supported");
  if (is_ascii(s->profile) && s->rc) return fail(SASSY_HIP_EUNSUPPORTED, "reverse complement is not defined for the ascii alphabet");
  if (n_patterns == 0) return fail(SASSY_HIP_EINVAL, std::string(who) + " needs at least one pattern");
  for (size_t i = 0; i < n_patterns; ++i) {
    if (!patterns[i] || pattern_lens[i] == 0) return fail(SASSY_HIP_EINVAL, "empty pattern (pattern " + std::to_string(i) + ")");
    if (!valid_pattern(s->profile, patterns[i], pattern_lens[i])) return fail(SASSY_HIP_EINVAL, "Pattern is not valid IUPAC");
  }
  if (k > 0x7FFFFFFFull) return fail(SASSY_HIP_EINVAL, "k is larger than 2^31 - 1");
  for (size_t i = 0; i < n_patterns; ++i) {
    if (pattern_lens[i] > kHamMaxRows)
      return fail(SASSY_HIP_EUNSUPPORTED, "the Hamming search takes patterns of at most " + std::to_string(kHamMaxRows) + " rows (pattern " +
                                              std::to_string(i) + " has " + std::to_string(pattern_lens[i]) + ")");
    if (is_ascii(s->profile)) {
      bool seen[256] = {};
      size_t distinct = 0;
      for (size_t j = 0; j < pattern_lens[i]; ++j) {
        const uint32_t c = s->profile == PROFILE_ASCII_CI ? fold_ascii(patterns[i][j]) : patterns[i][j];
        if (!seen[c]) { seen[c] = true; ++distinct; }
      }
      if (distinct > (size_t)kMaxSlots)
        return fail(SASSY_HIP_EUNSUPPORTED, "the Hamming search takes Ascii patterns of at most " + std::to_string(kMaxSlots) +
                                                " distinct bytes (pattern " + std::to_string(i) + " has " + std::to_string(distinct) + ")");
    }
  }
  SASSY_NO_TICKETS(s);
  return 0;
}

int hamming_family_refusals(sassy_SearcherType* s, const uint8_t* const* pats, const size_t* lens, size_t n_pats, size_t k, const char* who) {
  return hamming_refusals(s, pats, lens, n_pats, k, who);
}

// both batch entry points: out != nullptr the records, else the per-text outputs
static int hamming_many(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                        const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags, sassy_hip_Result** out,
                        uint8_t* out_cost, uint32_t* out_pattern, uint8_t* out_strand, uint64_t* out_start) {
  const bool best = out == nullptr;
  const char* who = best ? "hamming_best_pattern" : "search_hamming_many";
  if (!s || (!out && !out_cost) || (n_patterns && (!patterns || !pattern_lens)) || (n_texts && (!texts || !text_lens)))
    return fail(SASSY_HIP_EINVAL, std::string("Pointers in ") + who + "() must not be null");
  for (size_t t = 0; t < n_texts; ++t)
    if (!texts[t] && text_lens[t]) return fail(SASSY_HIP_EINVAL, std::string("Pointers in ") + who + "() must not be null (text " + std::to_string(t) + ")");
  if (flags & ~(uint32_t)(best ? 0u : SASSY_HIP_WITHOUT_TRACE))
    return fail(SASSY_HIP_EINVAL, best ? "hamming_best_pattern takes no flags (host texts only)"
                                       : "search_hamming_many takes SASSY_HIP_WITHOUT_TRACE only (host texts only)");
  if (best && k > 254) return fail(SASSY_HIP_EINVAL, "hamming_best_pattern: k must be <= 254 (costs are bytes, 255 = no match)");
  if (int rc = hamming_refusals(s, patterns, pattern_lens, n_patterns, k, who)) return rc;
  if (best) {  // what the device cell cannot hold
    if (n_patterns >= (1u << 23)) return fail(SASSY_HIP_EUNSUPPORTED, "hamming_best_pattern takes fewer than 2^23 patterns (the cell keeps 2 pattern + strand in 24 bits)");
    for (size_t t = 0; t < n_texts; ++t)
      if ((uint64_t)text_lens[t] >= (1ull << 32))
        return fail(SASSY_HIP_EUNSUPPORTED, "hamming_best_pattern takes texts shorter than 2^32 bytes (text " + std::to_string(t) + ": the cell keeps the start in 32 bits)");
  }
  sassy_hip_Result* R = best ? nullptr : new sassy_hip_Result();
  std::unique_ptr<sassy_hip_Result> owned(R);
  std::vector<unsigned long long> cells;
  if (n_texts) {
    DeviceGuard on_device(s);
    const double t0 = now_ms();
    reset_stats(s);
    if (int rc = s->ensure_device()) return rc;
    size_t longest = 0;
    for (size_t i = 0; i < n_patterns; ++i) longest = std::max(longest, pattern_lens[i]);
    const uint32_t kk = (uint32_t)std::min<size_t>(k, longest);  // k >= m reports every start
    if (best) cells.assign(n_texts, ~0ull);
    if (int rc = hamming_many_on_device(s, patterns, pattern_lens, n_patterns, texts, text_lens, n_texts, kk, (flags & SASSY_HIP_WITHOUT_TRACE) != 0,
                                        R, best ? cells.data() : nullptr)) {
      (void)hipStreamSynchronize(s->stream);
      return rc;
    }
    s->stats.total_ms = now_ms() - t0;
  }
  if (best) {
    for (size_t t = 0; t < n_texts; ++t) {
      const unsigned long long c = cells[t];
      const bool none = c == ~0ull;
      out_cost[t] = none ? (uint8_t)SASSY_HIP_NO_MATCH : (uint8_t)(c >> 56);
      if (out_pattern) out_pattern[t] = none ? 0xFFFFFFFFu : (uint32_t)((c >> 33) & 0x7FFFFFu);
      if (out_strand) out_strand[t] = none ? 0 : (uint8_t)((c >> 32) & 1u);
      if (out_start) out_start[t] = none ? UINT64_MAX : (uint64_t)(c & 0xFFFFFFFFull);
    }
    return 0;
  }
  if (R->pool.empty()) R->pool.push_back('\0');
  *out = owned.release();
  return 0;
}

// Copies of a counts table of n_bins counters (a power of two).  In the worst case -- every wavefront holds hits of one cost of
// one pattern -- every tile adds to one word, and a launch of few patterns streams tiles at the rate of HBM: 6.3 TB/s over 4 KiB
// tiles is about 1 500 adds per microsecond where one contended word takes about 88: 18 words are needed, 32
// are kept while 32 tables stay within 2^16 counters (512 KiB to clear and to read back), fewer for a larger table -- whose
// launches hold more patterns per tile and so add to one word less often --, one at least.  `forced` > 0: that many (option
// hamming_count_copies; rounded down to a power of two, at most 1024, within 2^26 counters).
static uint32_t hamming_count_copies(uint64_t n_bins, long forced) {
  uint32_t copies = 32;
  uint64_t room = 1ull << 16;
  if (forced > 0) {
    copies = 1;
    while (copies * 2 <= (uint64_t)std::min<long>(forced, 1024)) copies *= 2;
    room = 1ull << 26;
  }
  while (copies > 1 && (uint64_t)copies * n_bins > room) copies /= 2;
  return copies;
}

// both counting entry points: texts == nullptr the single text (text, text_len), else the batch
static int hamming_counts(sassy_SearcherType* s, const uint8_t* const* pats, const size_t* lens, size_t n_pats, const void* text,
                          size_t text_len, const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags,
                          uint64_t* out_counts, bool batch) {
  const char* who = batch ? "hamming_counts_many" : "hamming_counts";
  if (!s || !out_counts || (n_pats && (!pats || !lens)) || (!batch && !text && text_len) || (batch && n_texts && (!texts || !text_lens)))
    return fail(SASSY_HIP_EINVAL, std::string("Pointers in ") + who + "() must not be null");
  if (batch)
    for (size_t t = 0; t < n_texts; ++t)
      if (!texts[t] && text_lens[t])
        return fail(SASSY_HIP_EINVAL, std::string("Pointers in ") + who + "() must not be null (text " + std::to_string(t) + ")");
  if (batch && flags) return fail(SASSY_HIP_EINVAL, "hamming_counts_many takes no flags (host texts only)");
  if (flags & ~(uint32_t)(SASSY_HIP_TEXT_ON_DEVICE | SASSY_HIP_TEXT_UNCHANGED))
    return fail(SASSY_HIP_EINVAL, "hamming_counts takes SASSY_HIP_TEXT_ON_DEVICE and _TEXT_UNCHANGED only");
  if (k > 254) return fail(SASSY_HIP_EINVAL, std::string(who) + ": k must be <= 254 (the Hamming family's costs are bytes)");
  if (int rc = hamming_refusals(s, pats, lens, n_pats, k, who)) return rc;
  const uint64_t stride = (uint64_t)k + 1;
  if ((uint64_t)n_pats > 0xFFFFFFFFull / (2 * stride))
    return fail(SASSY_HIP_EUNSUPPORTED, std::string(who) + ": the table has more than 2^32 - 1 bins (" + std::to_string(n_pats) + " patterns x 2 x " +
                                            std::to_string(stride) + ")");
  const uint64_t n_bins = (uint64_t)n_pats * 2 * stride;
  std::fill(out_counts, out_counts + n_bins, (uint64_t)0);
  if (batch && n_texts == 0) return 0;
  DeviceGuard on_device(s);
  const double t0 = now_ms();
  reset_stats(s);
  if (int rc = s->ensure_device()) return rc;
  const uint32_t copies = hamming_count_copies(n_bins, s->sw.hamming_count_copies);
  if (int rc = s->d_ham_bins.reserve((size_t)copies * n_bins)) return rc;
  HIP_TRY(hipMemsetAsync(s->d_ham_bins.p, 0, (size_t)copies * n_bins * 8, s->stream));
  HamCounts C{};
  C.bins = s->d_ham_bins.p; C.n_bins = (uint32_t)n_bins; C.stride = (uint32_t)stride; C.copy_mask = copies - 1;
  size_t longest = 0;
  for (size_t i = 0; i < n_pats; ++i) longest = std::max(longest, lens[i]);
  const uint32_t kk = (uint32_t)std::min<size_t>(k, longest);  // k >= m counts every start
  int rc = 0;
  if (batch) {
    rc = hamming_many_on_device(s, pats, lens, n_pats, texts, text_lens, n_texts, kk, true, nullptr, nullptr, &C);
  } else {
    const uint8_t* d_text = static_cast<const uint8_t*>(text);
    if (flags & SASSY_HIP_TEXT_ON_DEVICE) {
      if (((uintptr_t)text & 15) != 0) return fail(SASSY_HIP_EINVAL, "device text pointer must be 16-byte aligned");
    } else if (text_len) {
      if (int rc2 = s->d_text.reserve(text_len + 64)) return rc2;
      HIP_TRY(hipMemcpyAsync(s->d_text.p, text, text_len, hipMemcpyHostToDevice, s->stream));
      d_text = s->d_text.p;
    }
    rc = hamming_on_device(s, pats, lens, n_pats, d_text, text_len, kk, true, nullptr, nullptr, &C);
  }
  if (rc) {
    (void)hipStreamSynchronize(s->stream);
    return rc;
  }
  // the copies come back once and are summed here
  std::vector<uint64_t> all((size_t)copies * n_bins);
  HIP_TRY(hipMemcpyAsync(all.data(), s->d_ham_bins.p, all.size() * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  uint64_t total = 0;
  for (uint32_t c = 0; c < copies; ++c)
    for (uint64_t b = 0; b < n_bins; ++b) out_counts[b] += all[(size_t)c * n_bins + b];
  for (uint64_t b = 0; b < n_bins; ++b) total += out_counts[b];
  s->stats.candidates = total;
  s->stats.filtered = 7;
  s->stats.blocks_per_chunk = kHamTileBlocks;
  s->stats.total_ms = now_ms() - t0;
  return 0;
}

}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_search_hamming(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                             const void* text, size_t text_len, size_t k, uint32_t flags, sassy_hip_Result** out) {
  if (!s || !out || (n_patterns && (!patterns || !pattern_lens)) || (!text && text_len))
    return fail(SASSY_HIP_EINVAL, "Pointers in search_hamming() must not be null");
  if (flags & ~(uint32_t)(SASSY_HIP_WITHOUT_TRACE | SASSY_HIP_TEXT_ON_DEVICE | SASSY_HIP_TEXT_UNCHANGED))
    return fail(SASSY_HIP_EINVAL, "search_hamming takes SASSY_HIP_WITHOUT_TRACE, _TEXT_ON_DEVICE and _TEXT_UNCHANGED only");
  if (int rc = hamming_refusals(s, patterns, pattern_lens, n_patterns, k, "search_hamming")) return rc;
  DeviceGuard on_device(s);
  const double t0 = now_ms();
  reset_stats(s);
  if (int rc = s->ensure_device()) return rc;
  const uint8_t* d_text = static_cast<const uint8_t*>(text);
  if (flags & SASSY_HIP_TEXT_ON_DEVICE) {
    if (((uintptr_t)text & 15) != 0) return fail(SASSY_HIP_EINVAL, "device text pointer must be 16-byte aligned");
  } else if (text_len) {
    if (int rc = s->d_text.reserve(text_len + 64)) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_text.p, text, text_len, hipMemcpyHostToDevice, s->stream));
    d_text = s->d_text.p;
  }
  sassy_hip_Result* R = new sassy_hip_Result();
  size_t longest = 0;
  for (size_t i = 0; i < n_patterns; ++i) longest = std::max(longest, pattern_lens[i]);
  const uint32_t kk = (uint32_t)std::min<size_t>(k, longest);  // k >= m reports every start
  if (int rc = hamming_on_device(s, patterns, pattern_lens, n_patterns, d_text, text_len, kk, (flags & SASSY_HIP_WITHOUT_TRACE) != 0, R)) {
    (void)hipStreamSynchronize(s->stream);
    delete R;
    return rc;
  }
  if (R->pool.empty()) R->pool.push_back('\0');
  s->stats.total_ms = now_ms() - t0;
  *out = R;
  return 0;
}

int sassy_hip_search_hamming_many(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                  const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags,
                                  sassy_hip_Result** out) {
  if (!out) return fail(SASSY_HIP_EINVAL, "Pointers in search_hamming_many() must not be null");
  return hamming_many(s, patterns, pattern_lens, n_patterns, texts, text_lens, n_texts, k, flags, out, nullptr, nullptr, nullptr, nullptr);
}

int sassy_hip_hamming_best_pattern(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                   const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags,
                                   uint8_t* out_cost, uint32_t* out_pattern, uint8_t* out_strand, uint64_t* out_start) {
  if (!out_cost && n_texts) return fail(SASSY_HIP_EINVAL, "Pointers in hamming_best_pattern() must not be null");
  uint8_t none = 0;
  return hamming_many(s, patterns, pattern_lens, n_patterns, texts, text_lens, n_texts, k, flags, nullptr, out_cost ? out_cost : &none,
                      out_pattern, out_strand, out_start);
}

int sassy_hip_hamming_counts(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                             const void* text, size_t text_len, size_t k, uint32_t flags, uint64_t* out_counts) {
  return hamming_counts(s, patterns, pattern_lens, n_patterns, text, text_len, nullptr, nullptr, 0, k, flags, out_counts, false);
}

int sassy_hip_hamming_counts_many(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                  const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags,
                                  uint64_t* out_counts) {
  return hamming_counts(s, patterns, pattern_lens, n_patterns, nullptr, 0, texts, text_lens, n_texts, k, flags, out_counts, true);
}

}  // extern "C"
