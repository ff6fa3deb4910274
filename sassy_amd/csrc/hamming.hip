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
//
// The host side, behind the kernels.  What needs no device is decided in hamming_plan.h (scanned patterns, launch groups, a
// group's tables and shape, the overflow step, text batches, count copies, the prefix).  Here:
//   ham_prepare / launch_range / ham_scan_range   a group's tables uploaded once; the one place that fills HamParams and
//                    launches; one range of tiles scanned until its items fit the list, sorted, on the host
//   ham_for_groups   the group loop of the three drivers: hamming_records (lists into a Result, ranges through
//                    ham_walk_ranges), hamming_cells (best pattern), hamming_add_counts -- each over one HamText, which is
//                    one device text or one laid-out batch
//   ham_for_text_batches   the _many calls: one loop over text batches that calls one of the three
//   hamming_refusals, hamming_count_call and the five entry points, each behind hamming_call (host_internal.h)
//   hamming_reads_records / _cells / _counts   the three drivers over a batch that is already resident and laid out (the
//                    handle of fastq_reads.hip, whose entry points call them)
#include "host_internal.h"
#include "profile_masks.h"
#include "hamming_step.h"

namespace sassy_hip {
namespace {

static_assert(kHamMaxHalo == (kHamMaxRows - 1 + 63) / 64, "halo of the longest pattern");
static_assert((uint32_t)PROFILE_DNA == kHamDna && (uint32_t)PROFILE_IUPAC == kHamIupac && (uint32_t)PROFILE_ASCII_CI == kHamAsciiCi,
              "hamming_step.h names the profiles by value");

// (HamItem, the pattern table's layout -- kHamTabWords, kHamNoFilter --, HamPattern, kHamStageBytes, kHamLdsBudget and
// ham_lds_per_wave: hamming_plan.h)

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

}  // namespace

// ---- the device side of the driver: prepare a group, launch a range, scan a range ----
int ham_prepare(sassy_SearcherType* S, const HamJob& J, HamPrepared& P) {
  ScanLane& L = S->lanes[0];
  P.t = ham_tables((uint32_t)S->profile, J.pats, J.np, J.group, S->sw.hamming_items);
  const HamTables& T = P.t;
  memcpy(P.SP.slot_val, J.group.slot_val, sizeof(J.group.slot_val));
  P.SP.nslots = J.group.ns;
  P.SP.profile = (uint32_t)S->profile;
  P.item_cap = T.item_cap;
  if (int rc = S->d_ham_tab.reserve(T.tab.size() + T.rows.size() + (T.pats.size() + 3) / 4 + 16)) return rc;
  P.d_tab = S->d_ham_tab.p;
  P.d_rows = P.d_tab + T.tab.size();
  P.d_pats = reinterpret_cast<uint8_t*>(P.d_rows + T.rows.size());
  if (int rc = S->d_ham_count.reserve(16)) return rc;
  L.h_up_used = 0;
  if (int rc = L.upload(P.d_tab, T.tab.data(), T.tab.size() * 4)) return rc;
  if (int rc = L.upload(P.d_rows, T.rows.data(), T.rows.size() * 4)) return rc;
  return L.upload(P.d_pats, T.pats.data(), T.pats.size());
}

namespace {
// Where a launch's hits go: into the item list, into the best-pattern cells of a batch's texts, or into a counts table.
struct HamSink {
  enum Kind { Items, Cells, Counts } kind;
  unsigned long long* cells;  // Cells: one per text of the batch (device)
  HamCounts counts;           // Counts
};

// One launch over tiles [tile0, tile0 + n_tiles) and the wait for it: the parameters, the event pair of a timed searcher, the
// stats lines.  Items: the list takes P.item_cap of them and *count is what the launch counted, which goes on past the list.
int launch_range(sassy_SearcherType* S, const HamJob& J, const HamPrepared& P, uint64_t tile0, uint64_t n_tiles, const HamSink& sink,
                 uint32_t* count) {
  hipStream_t st = S->stream;
  ScanLane& L = S->lanes[0];
  const bool timed = S->timing >= 1, list = sink.kind == HamSink::Items, many = J.text.starts != nullptr;
  HamParams H{};
  H.text = J.text.d_text; H.n = J.text.n; H.n_blocks = J.text.n_blocks(); H.tile0 = tile0; H.n_tiles = n_tiles;
  H.k = J.k; H.n_pat = J.np; H.halo = P.t.halo; H.nb = P.t.nb; H.n_filter = P.t.n_filter ? 1u : 0u;
  H.tab = P.d_tab; H.rows = P.d_rows;
  if (list) {
    H.item_cap = (uint32_t)P.item_cap; H.items = reinterpret_cast<HamItem*>(S->d_ham_items.p); H.item_count = S->d_ham_count.p;
    HIP_TRY(hipMemsetAsync(S->d_ham_count.p, 0, 4, st));
  }
  const HamMany M{J.text.rem, J.text.starts, J.text.n_texts, sink.cells};
  if (timed) HIP_TRY(hipEventRecord(L.ev_a, st));
  const uint32_t grid = (uint32_t)((n_tiles + P.t.wpg - 1) / P.t.wpg);
  HIP_TRY(launch_scan(S->profile, J.group.ns, H, P.SP, many ? &M : nullptr, sink.kind == HamSink::Counts ? &sink.counts : nullptr, grid,
                      P.t.wpg * 64, P.t.smem, st));
  if (timed) HIP_TRY(hipEventRecord(L.ev_b, st));
  if (list) HIP_TRY(hipMemcpyAsync(count, S->d_ham_count.p, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (the next group reuses the pinned upload area)
  if (timed) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, L.ev_a, L.ev_b) == hipSuccess) S->stats.scan_ms += ms;
  }
  S->stats.scan_launches += 1;
  S->stats.grid = grid;
  return 0;
}
}  // namespace

// One range of a prepared group's tiles, from tile0 to the text's end or as far as the item list holds: the scan, the step
// after an overflow (hamming_plan.h) and the launch again, the sort by (pattern | strand, block), the items on the host.
int ham_scan_range(sassy_SearcherType* S, const HamJob& J, HamPrepared& P, uint64_t tile0, HamRangeOut& out) {
  hipStream_t st = S->stream;
  const uint64_t n_blocks = J.text.n_blocks();
  uint64_t span = std::min(J.text.n_tiles() - tile0, P.t.span_max);
  uint32_t count = 0;
  out = HamRangeOut{};
  while (!out.overflow) {
    if (int rc = S->d_ham_items.reserve(P.item_cap)) return rc;
    if (int rc = launch_range(S, J, P, tile0, span, HamSink{HamSink::Items, nullptr, {}}, &count)) return rc;
    const HamStep step = ham_overflow_step(count, P.item_cap, P.t.max_cap, span, J.min_span);
    P.item_cap = step.item_cap;
    span = step.span;
    if (step.what == HamStep::Done) break;
    out.overflow = step.what == HamStep::Overflow;
  }
  out.span = span;
  out.count = count;
  if (out.overflow) return 0;
  S->stats.blocks += std::min<uint64_t>(span * kHamTileBlocks, n_blocks - tile0 * kHamTileBlocks);
  S->stats.hit_blocks += count;
  if (count) {
    if (int rc = S->d_ham_sorted.reserve(count)) return rc;
    if (int rc = S->d_ham_sort.reserve(sort_scratch_bytes(count))) return rc;
    int key_bits = 33;
    while (key_bits < 64 && ((uint64_t)(J.np - 1) >> (key_bits - 32)) != 0) ++key_bits;
    HIP_TRY(launch_sort_candidates(S->d_ham_items.p, S->d_ham_sorted.p, count, S->d_ham_sort.p, S->d_ham_sort.cap, st, 0, key_bits));
    out.items.resize(count);
    HIP_TRY(hipMemcpyAsync(out.items.data(), S->d_ham_sorted.p, (size_t)count * sizeof(HamItem), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return 0;
}

namespace {
// ---- the three drivers: refusals are the caller's ----
// The loop over launch groups that they share: the patterns as scanned, cut into groups, every group prepared once and
// handed to per_group(J, P), which scans the whole text.
template <typename PerGroup>
int ham_for_groups(sassy_SearcherType* S, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns, const HamText& text,
                   uint32_t k, PerGroup&& per_group) {
  const Profile pr = S->profile;
  if (text.n_blocks() + kHamMaxHalo > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "text too long for the Hamming search (2^32 blocks)");
  S->stats.filtered = 7;
  S->stats.blocks_per_chunk = kHamTileBlocks;
  const std::vector<HamPattern> all = ham_scanned_patterns(patterns, pattern_lens, n_patterns, S->rc, S->max_n_frac, text.longest,
                                                           [pr](uint8_t c) { return complement_char(pr, c); });
  const size_t max_batch = ham_batch_patterns(S->sw.hamming_batch);
  for (size_t a0 = 0; a0 < all.size();) {
    HamJob J;
    J.group = ham_next_group((uint32_t)pr, all, a0, max_batch);
    J.pats = &all[a0]; J.np = (uint32_t)(J.group.a1 - a0);
    J.text = text; J.k = k;
    HamPrepared P;
    if (int rc = ham_prepare(S, J, P)) return rc;
    if (int rc = per_group(J, P)) return rc;
    S->stats.text_bytes += text.n;
    a0 = J.group.a1;
  }
  S->stats.chunks = text.n_tiles();
  return 0;
}

// the contract's order of records as far as groups, ranges and batches disturb it: a stable sort on it restores the rest
bool by_pattern(const sassy_hip_Match& a, const sassy_hip_Match& b) {
  return a.pattern_idx != b.pattern_idx ? a.pattern_idx < b.pattern_idx : a.strand < b.strand;
}

// List records into R: the text in ranges of tiles, every range's hits emitted in batches of the record block.
int hamming_records(sassy_SearcherType* S, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns, const HamText& text,
                    uint32_t k, bool without_trace, sassy_hip_Result* R) {
  hipStream_t st = S->stream;
  ScanLane& L = S->lanes[0];
  return ham_for_groups(S, patterns, pattern_lens, n_patterns, text, k, [&](const HamJob& J, HamPrepared& P) {
    const size_t first_row = R->matches.size();
    auto per_range = [&](const HamRangeOut& range, uint64_t, bool, uint64_t*) {
      if (range.count == 0) return 0;
      std::vector<uint32_t> prefix;
      uint64_t hits = 0;
      if (!ham_prefix(range.items, R->matches.size(), prefix, &hits))
        return fail(SASSY_HIP_ENOMEM, "Hamming search: more than 2^32 records (" + std::to_string(R->matches.size() + hits) + ")");
      if (int rc = S->d_ham_prefix.reserve(range.count)) return rc;
      HIP_TRY(hipMemcpyAsync(S->d_ham_prefix.p, prefix.data(), (size_t)range.count * 4, hipMemcpyHostToDevice, st));
      const uint32_t stride = without_trace ? 0u : 2u * P.t.longest + 8u;
      std::vector<MatchOut> rows_h;
      std::vector<char> strs_h;
      auto reserve = [&](uint64_t batch) {
        if (int rc = L.d_trace.reserve(batch)) return rc;
        return stride ? L.d_str.reserve(batch * stride) : 0;
      };
      auto emit = [&](uint64_t r0, uint32_t cnt) {
        EmitParams E{};
        E.text = text.d_text; E.items = reinterpret_cast<const HamItem*>(S->d_ham_sorted.p); E.prefix = S->d_ham_prefix.p; E.n_items = range.count;
        E.first = (uint32_t)r0; E.count = cnt; E.tab = P.d_tab; E.pats = P.d_pats; E.profile = (uint32_t)S->profile; E.str_stride = stride;
        E.out = L.d_trace.p; E.strs = reinterpret_cast<char*>(L.d_str.p);
        E.starts = text.starts; E.n_texts = text.n_texts; E.text0 = text.text0;
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
          if (R->pool.size() + mo.cigar_len + 1 > 0xFFFFFFFFull) return fail(SASSY_HIP_ENOMEM, "Hamming search: more than 4 GiB of cigar text");
          const uint32_t off = (uint32_t)R->pool.size();
          if (stride) R->pool.append(strs_h.data() + (size_t)i * stride, mo.cigar_len);
          R->pool.push_back('\0');
          mo.cigar_off = off;
          R->matches.push_back(mo);
        }
        return 0;
      };
      if (int rc = ham_emit_batches(S, hits, reserve, emit)) return rc;
      S->stats.candidates += hits;
      return 0;
    };
    return ham_walk_ranges(S, J, P, per_range, [&] { std::stable_sort(R->matches.begin() + (long)first_row, R->matches.end(), by_pattern); });
  });
}

// Reduce into cells, or add into a counts table: nothing is listed, one launch per group takes every tile.
int hamming_into(sassy_SearcherType* S, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns, const HamText& text,
                 uint32_t k, const HamSink& sink) {
  return ham_for_groups(S, patterns, pattern_lens, n_patterns, text, k, [&](const HamJob& J, HamPrepared& P) {
    if (int rc = launch_range(S, J, P, 0, text.n_tiles(), sink, nullptr)) return rc;
    S->stats.blocks += text.n_blocks();
    return 0;
  });
}
// per text of the batch its best-pattern cell (device; all ones: no hit)
int hamming_cells(sassy_SearcherType* S, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns, const HamText& batch,
                  uint32_t k, unsigned long long* d_cells) {
  return hamming_into(S, patterns, pattern_lens, n_patterns, batch, k, HamSink{HamSink::Cells, d_cells, {}});
}
int hamming_add_counts(sassy_SearcherType* S, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns, const HamText& text,
                       uint32_t k, const HamCounts& C) {
  return hamming_into(S, patterns, pattern_lens, n_patterns, text, k, HamSink{HamSink::Counts, nullptr, C});
}

// A batch call: the texts in batches of at most `hamming_many_batch` bytes (hamming_plan.h) laid out and uploaded, rem[] built
// on the device, every batch handed to per_batch(text, t0, nt) -- one of the three drivers over texts [t0, t0 + nt) of the call.
template <typename PerBatch>
int ham_for_text_batches(sassy_SearcherType* S, const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, PerBatch&& per_batch) {
  hipStream_t st = S->stream;
  const uint64_t batch_cap = ham_many_batch_bytes(S->sw.hamming_many_batch);
  uint64_t all_tiles = 0;
  for (size_t t0 = 0; t0 < n_texts;) {
    const HamTextBatch B = ham_next_text_batch(text_lens, n_texts, t0, batch_cap);
    const size_t nt = B.t1 - t0;
    const uint64_t total = B.total, n_blocks = total / 64;
    t0 = B.t1;
    if (nt > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "Hamming search: more than 2^32 texts in one batch");
    if (total == 0) continue;  // (only empty texts: no hits)
    if (int rc = S->reserve_stage(total + 64)) return rc;
    if (int rc = S->d_text.reserve(total + 64)) return rc;
    if (int rc = layout_and_upload(S->h_stage, S->d_text.p, texts + B.t0, text_lens + B.t0, B.start.data(), nt, total, (uint8_t)0, st)) return rc;
    if (int rc = S->d_ham_texts.reserve(2 * nt)) return rc;
    if (int rc = S->d_ham_rem.reserve(n_blocks)) return rc;
    HIP_TRY(hipMemcpyAsync(S->d_ham_texts.p, B.start.data(), nt * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S->d_ham_texts.p + nt, B.len.data(), nt * 8, hipMemcpyHostToDevice, st));
    if (n_blocks + 255 > 0xFFFFFFFFull * 256ull) return fail(SASSY_HIP_EUNSUPPORTED, "text batch too long for the Hamming search");
    hipLaunchKernelGGL(ham_rem_kernel, dim3((uint32_t)((n_blocks + 255) / 256)), dim3(256), 0, st, S->d_ham_texts.p, S->d_ham_texts.p + nt,
                       (uint32_t)nt, n_blocks, S->d_ham_rem.p);
    HIP_TRY(hipGetLastError());
    HamText text;
    text.d_text = S->d_text.p; text.n = total; text.longest = B.longest;
    text.rem = S->d_ham_rem.p; text.starts = S->d_ham_texts.p; text.n_texts = (uint32_t)nt; text.text0 = B.t0;
    if (int rc = per_batch(text, B.t0, nt)) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // (the tables of the next batch overwrite this one's)
    all_tiles += S->stats.chunks;
  }
  S->stats.chunks = all_tiles;
  S->stats.filtered = 7;
  S->stats.blocks_per_chunk = kHamTileBlocks;
  return 0;
}

// ---- what the entry points share ----
// the pointers of a batch call; have_out: its output pointers are there
int many_pointers(const sassy_SearcherType* s, bool have_out, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                  const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, const char* who) {
  if (!s || !have_out || (n_patterns && (!patterns || !pattern_lens)) || (n_texts && (!texts || !text_lens)))
    return fail(SASSY_HIP_EINVAL, std::string("Pointers in ") + who + "() must not be null");
  for (size_t t = 0; t < n_texts; ++t)
    if (!texts[t] && text_lens[t]) return fail(SASSY_HIP_EINVAL, std::string("Pointers in ") + who + "() must not be null (text " + std::to_string(t) + ")");
  return 0;
}

// Both counting entry points behind their pointer and flag checks: the refusals, the table cleared, scan(k, C) -- the driver
// over the one text or over the batches -- between the table's copies on the device and their sum in out_counts.
template <typename Scan>
int hamming_count_call(sassy_SearcherType* s, const uint8_t* const* pats, const size_t* lens, size_t n_pats, size_t k, const char* who,
                       bool nothing_to_scan, uint64_t* out_counts, Scan&& scan) {
  if (k > 254) return fail(SASSY_HIP_EINVAL, std::string(who) + ": k must be <= 254 (the Hamming family's costs are bytes)");
  if (int rc = hamming_refusals(s, pats, lens, n_pats, k, who)) return rc;
  const uint64_t stride = (uint64_t)k + 1;
  if ((uint64_t)n_pats > 0xFFFFFFFFull / (2 * stride))
    return fail(SASSY_HIP_EUNSUPPORTED, std::string(who) + ": the table has more than 2^32 - 1 bins (" + std::to_string(n_pats) + " patterns x 2 x " +
                                            std::to_string(stride) + ")");
  const uint64_t n_bins = (uint64_t)n_pats * 2 * stride;
  std::fill(out_counts, out_counts + n_bins, (uint64_t)0);
  if (nothing_to_scan) return 0;
  return hamming_call(s, lens, n_pats, k, [&](uint32_t kk) {
    const uint32_t copies = hamming_count_copies(n_bins, s->sw.hamming_count_copies);
    if (int rc = s->d_ham_bins.reserve((size_t)copies * n_bins)) return rc;
    HIP_TRY(hipMemsetAsync(s->d_ham_bins.p, 0, (size_t)copies * n_bins * 8, s->stream));
    HamCounts C{};
    C.bins = s->d_ham_bins.p; C.n_bins = (uint32_t)n_bins; C.stride = (uint32_t)stride; C.copy_mask = copies - 1;
    if (int rc = scan(kk, C)) return rc;
    // the copies come back once and are summed here
    std::vector<uint64_t> all((size_t)copies * n_bins);
    HIP_TRY(hipMemcpyAsync(all.data(), s->d_ham_bins.p, all.size() * 8, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    uint64_t total = 0;
    for (uint32_t c = 0; c < copies; ++c)
      for (uint64_t b = 0; b < n_bins; ++b) out_counts[b] += all[(size_t)c * n_bins + b];
    for (uint64_t b = 0; b < n_bins; ++b) total += out_counts[b];
    s->stats.candidates = total;
    return 0;
  });
}

}  // namespace

// What every Hamming entry point refuses, before any device work; `who` names the entry point.
int hamming_refusals(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns, size_t k,
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

// ---- a resident read batch (fastq_reads.hip): the three drivers over one HamText that is already laid out on the device,
// behind the caller's pointer and flag checks.  No upload, no layout, no ham_rem_kernel; `device`: where the batch was made.
namespace {
int same_device(const sassy_SearcherType* s, int device, const char* who) {
  if (s->device == device) return 0;
  return fail(SASSY_HIP_EINVAL, std::string(who) + ": the reads were made on device " + std::to_string(device) + ", the searcher is on device " +
                                    std::to_string(s->device));
}
}  // namespace
// records into R, in the contract's order; the caller has called hamming_refusals
int hamming_reads_records(sassy_SearcherType* s, const uint8_t* const* pats, const size_t* lens, size_t n_pats, const HamText& reads, int device,
                          size_t k, bool without_trace, sassy_hip_Result* R) {
  return hamming_call(s, lens, n_pats, k, [&](uint32_t kk) {
    if (int rc = same_device(s, device, "search_hamming_reads")) return rc;
    if (reads.n == 0) return 0;  // (only empty reads: no hits)
    if (int rc = hamming_records(s, pats, lens, n_pats, reads, kk, without_trace, R)) return rc;
    // pattern groups and ranges each came in the contract's order: a stable sort on (pattern, strand) restores it for the call
    if (!std::is_sorted(R->matches.begin(), R->matches.end(), by_pattern)) std::stable_sort(R->matches.begin(), R->matches.end(), by_pattern);
    return 0;
  });
}
// per read its best-pattern cell, on the host (all ones: no hit); the caller has called hamming_refusals
int hamming_reads_cells(sassy_SearcherType* s, const uint8_t* const* pats, const size_t* lens, size_t n_pats, const HamText& reads, int device,
                        size_t k, unsigned long long* cells) {
  return hamming_call(s, lens, n_pats, k, [&](uint32_t kk) {
    if (int rc = same_device(s, device, "hamming_best_pattern_reads")) return rc;
    if (reads.n == 0) return 0;
    const size_t nt = reads.n_texts;
    if (int rc = s->d_ham_cells.reserve(nt)) return rc;
    HIP_TRY(hipMemsetAsync(s->d_ham_cells.p, 0xFF, nt * 8, s->stream));
    if (int rc = hamming_cells(s, pats, lens, n_pats, reads, kk, s->d_ham_cells.p)) return rc;
    HIP_TRY(hipMemcpyAsync(cells, s->d_ham_cells.p, nt * 8, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
  });
}
// the counts table; the refusals are hamming_count_call's
int hamming_reads_counts(sassy_SearcherType* s, const uint8_t* const* pats, const size_t* lens, size_t n_pats, const HamText& reads, int device,
                         size_t k, const char* who, uint64_t* out_counts) {
  return hamming_count_call(s, pats, lens, n_pats, k, who, reads.n_texts == 0, out_counts, [&](uint32_t kk, const HamCounts& C) {
    if (int rc = same_device(s, device, who)) return rc;
    if (reads.n == 0) return 0;
    return hamming_add_counts(s, pats, lens, n_pats, reads, kk, C);
  });
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
  return hamming_call(s, pattern_lens, n_patterns, k, [&](uint32_t kk) {
    HamText one;
    if (int rc = ham_one_text(s, text, text_len, flags, &one)) return rc;
    std::unique_ptr<sassy_hip_Result> R(new sassy_hip_Result());
    if (int rc = hamming_records(s, patterns, pattern_lens, n_patterns, one, kk, (flags & SASSY_HIP_WITHOUT_TRACE) != 0, R.get())) return rc;
    if (R->pool.empty()) R->pool.push_back('\0');
    *out = R.release();
    return 0;
  });
}

int sassy_hip_search_hamming_many(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                  const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags,
                                  sassy_hip_Result** out) {
  const char* who = "search_hamming_many";
  if (int rc = many_pointers(s, out != nullptr, patterns, pattern_lens, n_patterns, texts, text_lens, n_texts, who)) return rc;
  if (flags & ~(uint32_t)SASSY_HIP_WITHOUT_TRACE)
    return fail(SASSY_HIP_EINVAL, "search_hamming_many takes SASSY_HIP_WITHOUT_TRACE only (host texts only)");
  if (int rc = hamming_refusals(s, patterns, pattern_lens, n_patterns, k, who)) return rc;
  std::unique_ptr<sassy_hip_Result> R(new sassy_hip_Result());
  auto all_batches = [&](uint32_t kk) {
    if (int rc = ham_for_text_batches(s, texts, text_lens, n_texts, [&](const HamText& batch, size_t, size_t) {
          return hamming_records(s, patterns, pattern_lens, n_patterns, batch, kk, (flags & SASSY_HIP_WITHOUT_TRACE) != 0, R.get());
        }))
      return rc;
    // batches, pattern groups and ranges each came in the contract's order, and all of them ascend in text order: a stable
    // sort on (pattern, strand) restores it for the call
    if (!std::is_sorted(R->matches.begin(), R->matches.end(), by_pattern)) std::stable_sort(R->matches.begin(), R->matches.end(), by_pattern);
    return 0;
  };
  if (n_texts)
    if (int rc = hamming_call(s, pattern_lens, n_patterns, k, all_batches)) return rc;
  if (R->pool.empty()) R->pool.push_back('\0');
  *out = R.release();
  return 0;
}

int sassy_hip_hamming_best_pattern(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                   const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags,
                                   uint8_t* out_cost, uint32_t* out_pattern, uint8_t* out_strand, uint64_t* out_start) {
  const char* who = "hamming_best_pattern";
  if (int rc = many_pointers(s, out_cost || !n_texts, patterns, pattern_lens, n_patterns, texts, text_lens, n_texts, who)) return rc;
  if (flags) return fail(SASSY_HIP_EINVAL, "hamming_best_pattern takes no flags (host texts only)");
  if (k > 254) return fail(SASSY_HIP_EINVAL, "hamming_best_pattern: k must be <= 254 (costs are bytes, 255 = no match)");
  if (int rc = hamming_refusals(s, patterns, pattern_lens, n_patterns, k, who)) return rc;
  // what the device cell cannot hold
  if (n_patterns >= (1u << 23)) return fail(SASSY_HIP_EUNSUPPORTED, "hamming_best_pattern takes fewer than 2^23 patterns (the cell keeps 2 pattern + strand in 24 bits)");
  for (size_t t = 0; t < n_texts; ++t)
    if ((uint64_t)text_lens[t] >= (1ull << 32))
      return fail(SASSY_HIP_EUNSUPPORTED, "hamming_best_pattern takes texts shorter than 2^32 bytes (text " + std::to_string(t) + ": the cell keeps the start in 32 bits)");
  if (n_texts == 0) return 0;
  std::vector<unsigned long long> cells(n_texts, ~0ull);
  auto all_batches = [&](uint32_t kk) {
    return ham_for_text_batches(s, texts, text_lens, n_texts, [&](const HamText& batch, size_t t0, size_t nt) {
      if (int rc = s->d_ham_cells.reserve(nt)) return rc;
      HIP_TRY(hipMemsetAsync(s->d_ham_cells.p, 0xFF, nt * 8, s->stream));
      if (int rc = hamming_cells(s, patterns, pattern_lens, n_patterns, batch, kk, s->d_ham_cells.p)) return rc;
      HIP_TRY(hipMemcpyAsync(cells.data() + t0, s->d_ham_cells.p, nt * 8, hipMemcpyDeviceToHost, s->stream));
      return 0;
    });
  };
  if (int rc = hamming_call(s, pattern_lens, n_patterns, k, all_batches)) return rc;
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

int sassy_hip_hamming_counts(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                             const void* text, size_t text_len, size_t k, uint32_t flags, uint64_t* out_counts) {
  if (!s || !out_counts || (n_patterns && (!patterns || !pattern_lens)) || (!text && text_len))
    return fail(SASSY_HIP_EINVAL, "Pointers in hamming_counts() must not be null");
  if (flags & ~(uint32_t)(SASSY_HIP_TEXT_ON_DEVICE | SASSY_HIP_TEXT_UNCHANGED))
    return fail(SASSY_HIP_EINVAL, "hamming_counts takes SASSY_HIP_TEXT_ON_DEVICE and _TEXT_UNCHANGED only");
  return hamming_count_call(s, patterns, pattern_lens, n_patterns, k, "hamming_counts", false, out_counts, [&](uint32_t kk, const HamCounts& C) {
    HamText one;
    if (int rc = ham_one_text(s, text, text_len, flags, &one)) return rc;
    return hamming_add_counts(s, patterns, pattern_lens, n_patterns, one, kk, C);
  });
}

int sassy_hip_hamming_counts_many(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                  const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags,
                                  uint64_t* out_counts) {
  const char* who = "hamming_counts_many";
  if (int rc = many_pointers(s, out_counts != nullptr, patterns, pattern_lens, n_patterns, texts, text_lens, n_texts, who)) return rc;
  if (flags) return fail(SASSY_HIP_EINVAL, "hamming_counts_many takes no flags (host texts only)");
  return hamming_count_call(s, patterns, pattern_lens, n_patterns, k, who, n_texts == 0, out_counts, [&](uint32_t kk, const HamCounts& C) {
    return ham_for_text_batches(s, texts, text_lens, n_texts, [&](const HamText& batch, size_t, size_t) {
      return hamming_add_counts(s, patterns, pattern_lens, n_patterns, batch, kk, C);
    });
  });
}

}  // extern "C"
