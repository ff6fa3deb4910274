// fasta_unwrap.hip -- a chunk of FASTA, raw bytes in, search-ready text out: records found, headers and line ends dropped,
// every record's sequence laid out from a multiple of 64 bytes on, all on the device (sassy_hip_fasta_unwrap).
//
// The definition and the bit arithmetic are in fasta_step.h.  Geometry as line_index.hip: a tile = 4 KiB = what one wavefront
// holds in registers, 64 consecutive bytes per lane (the masks need the bytes in order), 16-byte loads; a super-tile = 16
// tiles = what one workgroup of the count pass reads.  Launches:
//   fasta_count_kernel    reads the raw bytes once; per tile the summary (FastaSum) of the tiles in front of it INSIDE its
//                         super-tile, per super-tile its own summary
//   fasta_scan_kernel     one workgroup: the ordered scan of the super-tile summaries, 64-bit; in front of every super-tile
//                         the kept bytes, the header starts and the carried state; entry n_super = the totals  -> host
//   fasta_record_kernel   visits only tiles that hold a header start or begin inside a header line: per record the position of
//                         its '>', the end of its header line and the kept bytes in front of it
//   fasta_rec_sum_kernel, fasta_rec_top_kernel   the exclusive scan of the sequence lengths rounded up to 64 -> seq_start, in
//                         blocks of 1024 records and one workgroup over the block sums; the layout's size  -> host
//   fasta_rec_write_kernel  the record table (id_start, id_len, seq_start, seq_len) and the zero pad behind every sequence
//   fasta_compact_kernel  reads the raw bytes again: every lane stores its kept bytes from its registers at their ranks in an
//                         LDS image of the tile, which goes to seq_start[rec] + (kept in front of the byte - kept in front
//                         of rec).  A tile without a header start (nearly every tile of a genome) is one contiguous run:
//                         16-byte stores between its unaligned ends.
// Two host waits size what cannot be sized before: the record arrays (record count) and the text (layout bytes).
#include "host_internal.h"
#include "fasta_step.h"

struct sassy_hip_Fasta {
  std::vector<sassy_hip_FastaRecord> records;
  uint8_t* d_text = nullptr;
  uint64_t text_bytes = 0;  // the layout and the 64 spare bytes behind it
  int device = -1;
};

namespace sassy_hip {

namespace {

constexpr uint32_t kTile = kFaTileBytes;
constexpr uint32_t kTilesPerSuper = 16;
constexpr uint64_t kSuper = (uint64_t)kTile * kTilesPerSuper;
constexpr uint64_t kMaxSuper = 0x7FFFFFFFull;  // a grid's width; DESIGN 10
constexpr uint32_t kRecPerThread = 4, kRecBlock = 256 * kRecPerThread;
static_assert(kTile == 64 * kFaLaneBytes, "a tile is 64 lanes x 64 bytes");

// In front of a super-tile, from the input's first byte (which is a line start): resolved, no summary needed.
struct SuperPre {
  unsigned long long kept, hdr, state;  // state: the line open at the super-tile's first byte is a header
};

// bit b of the result: byte b of v equals the byte that c4 repeats four times (line_index.hip's newline test, for any byte)
__device__ __forceinline__ uint32_t eq_bits4(uint32_t v, uint32_t c4) {
  const uint32_t z = v ^ c4;
  const uint32_t t = ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;  // bit 7 of every zero byte of z, exactly
  return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}
__device__ __forceinline__ uint64_t eq_bits64(const uint4 (&v)[4], uint32_t c4) {
  uint64_t m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t b = eq_bits4(v[j].x, c4) | eq_bits4(v[j].y, c4) << 4 | eq_bits4(v[j].z, c4) << 8 | eq_bits4(v[j].w, c4) << 12;
    m |= (uint64_t)b << (16 * j);
  }
  return m;
}

// The lane's 64 bytes of a tile.  raw is 16-byte aligned and readable up to the next multiple of 64 behind n, so a 16-byte
// load that starts in front of n is legal.
__device__ __forceinline__ void load_lane(const uint8_t* raw, uint64_t n, uint64_t base, uint4 (&v)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = make_uint4(0u, 0u, 0u, 0u);
    if (base + 16u * j < n) v[j] = *reinterpret_cast<const uint4*>(raw + base + 16u * j);
  }
}

// The lane's masks; every lane of the wavefront calls this (shuffles).  *nl_out: its newline mask.
__device__ __forceinline__ FastaLane lane_masks(const uint4 (&v)[4], const uint8_t* raw, uint64_t n, uint64_t tile_base, uint32_t lane,
                                                uint64_t* nl_out, uint32_t* len_out) {
  const uint64_t base = tile_base + 64ull * lane;
  const uint32_t len = base >= n ? 0u : (uint32_t)min((uint64_t)64, n - base);
  const uint64_t valid = fa_below(len);
  const uint64_t nl = eq_bits64(v, 0x0A0A0A0Au) & valid, gt = eq_bits64(v, 0x3E3E3E3Eu) & valid, cr = eq_bits64(v, 0x0D0D0D0Du) & valid;
  const uint32_t last_nl = (uint32_t)(nl >> 63), first_end = len == 0 ? 1u : (uint32_t)(nl & 1ull);
  uint32_t prev = __shfl_up(last_nl, 1, 64), next = __shfl_down(first_end, 1, 64);
  if (lane == 0) prev = tile_base == 0 ? 1u : (raw[tile_base - 1] == 0x0A ? 1u : 0u);
  if (lane == 63) {
    const uint64_t q = tile_base + kTile;
    next = q >= n ? 1u : (raw[q] == 0x0A ? 1u : 0u);
  }
  *nl_out = nl;
  *len_out = len;
  return fa_lane(nl, gt, cr, len, prev != 0, next != 0);
}

// summaries through shuffles and global memory: flags = has_ls | last_hdr << 1; inside a tile both kept counts fit 16 bits
__device__ __forceinline__ FastaSum shfl_sum(const FastaSum& s, int o, bool up) {
  const uint32_t f = s.has_ls | s.last_hdr << 1, k = s.kept_pre | s.kept_post << 16;
  const uint32_t f2 = up ? __shfl_up(f, o, 64) : __shfl_down(f, o, 64);
  const uint32_t k2 = up ? __shfl_up(k, o, 64) : __shfl_down(k, o, 64);
  const uint32_t h2 = up ? __shfl_up(s.n_hdr, o, 64) : __shfl_down(s.n_hdr, o, 64);
  return FastaSum{f2 & 1u, (f2 >> 1) & 1u, k2 & 0xFFFFu, k2 >> 16, h2};
}
// the ordered sum of the wavefront's summaries, valid in lane 0
__device__ __forceinline__ FastaSum wave_reduce(FastaSum s) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s = fa_combine(s, shfl_sum(s, o, false));
  return s;
}
// excl: the lanes in front of this one; total (every lane): all 64
__device__ __forceinline__ void wave_scan(const FastaSum& mine, uint32_t lane, FastaSum* excl, FastaSum* total) {
  FastaSum incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const FastaSum up = shfl_sum(incl, o, true);
    if ((int)lane >= o) incl = fa_combine(up, incl);
  }
  const uint32_t f = incl.has_ls | incl.last_hdr << 1;
  const uint32_t tf = __shfl(f, 63, 64);
  *total = FastaSum{tf & 1u, (tf >> 1) & 1u, (uint32_t)__shfl(incl.kept_pre, 63, 64), (uint32_t)__shfl(incl.kept_post, 63, 64),
                    (uint32_t)__shfl(incl.n_hdr, 63, 64)};
  // (a lane's inclusive kept counts may reach 4096 = 0x1000: 16 bits hold them)
  const FastaSum up = shfl_sum(incl, 1, true);
  *excl = lane == 0 ? fa_identity<uint32_t>() : up;
}

// x: has_ls | last_hdr << 1 | (tile_pre only) the tile's OWN header starts << 2
__device__ __forceinline__ uint4 pack_sum(const FastaSum& s, uint32_t own_hdr) {
  return make_uint4(s.has_ls | s.last_hdr << 1 | own_hdr << 2, s.kept_pre, s.kept_post, s.n_hdr);
}
__device__ __forceinline__ FastaSum unpack_sum(const uint4 p) { return FastaSum{p.x & 1u, (p.x >> 1) & 1u, p.y, p.z, p.w}; }

// Pass one: a workgroup per super-tile, a wave per four of its tiles.
__global__ __launch_bounds__(256) void fasta_count_kernel(const uint8_t* raw, uint64_t n, uint64_t n_tiles, uint4* tile_pre, uint4* super_sum) {
  __shared__ FastaSum sums[kTilesPerSuper];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t tile0 = (uint64_t)blockIdx.x * kTilesPerSuper;
  for (uint32_t i = 0; i < kTilesPerSuper / 4; ++i) {
    const uint32_t t = wave * (kTilesPerSuper / 4) + i;
    FastaSum s = fa_identity<uint32_t>();
    if (tile0 + t < n_tiles) {  // (the same in every lane of the wave)
      uint4 v[4];
      load_lane(raw, n, (tile0 + t) * kTile + 64ull * lane, v);
      uint64_t nl;
      uint32_t len;
      const FastaLane L = lane_masks(v, raw, n, (tile0 + t) * kTile, lane, &nl, &len);
      s = wave_reduce(fa_summary(L));
    }
    if (lane == 0) sums[t] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    FastaSum run = fa_identity<uint32_t>();
    for (uint32_t t = 0; t < kTilesPerSuper; ++t) {
      if (tile0 + t < n_tiles) tile_pre[tile0 + t] = pack_sum(run, sums[t].n_hdr);
      run = fa_combine(run, sums[t]);
    }
    super_sum[blockIdx.x] = pack_sum(run, 0);
  }
}

// The ordered exclusive scan of the super-tile summaries: one workgroup, a contiguous run of entries per thread.
// super_pre has n_super + 1 entries.
__global__ __launch_bounds__(1024) void fasta_scan_kernel(const uint4* super_sum, uint64_t n_super, SuperPre* super_pre) {
  __shared__ FastaSum64 sums[1024];
  const uint64_t per = (n_super + 1023) / 1024;
  const uint64_t lo = min((uint64_t)threadIdx.x * per, n_super), hi = min(lo + per, n_super);
  FastaSum64 mine = fa_identity<uint64_t>();
  for (uint64_t i = lo; i < hi; ++i) mine = fa_combine(mine, unpack_sum(super_sum[i]));
  sums[threadIdx.x] = mine;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {  // Hillis-Steele, inclusive, in order
    const FastaSum64 front = threadIdx.x >= o ? sums[threadIdx.x - o] : fa_identity<uint64_t>();
    __syncthreads();
    sums[threadIdx.x] = fa_combine(front, sums[threadIdx.x]);
    __syncthreads();
  }
  FastaSum64 run = threadIdx.x ? sums[threadIdx.x - 1] : fa_identity<uint64_t>();
  for (uint64_t i = lo; i < hi; ++i) {
    super_pre[i] = SuperPre{fa_kept_total(run, false), run.n_hdr, fa_state_out(run, false) ? 1ull : 0ull};
    run = fa_combine(run, unpack_sum(super_sum[i]));
  }
  if (threadIdx.x == 1023) {
    const FastaSum64 all = sums[1023];
    super_pre[n_super] = SuperPre{fa_kept_total(all, false), all.n_hdr, fa_state_out(all, false) ? 1ull : 0ull};
  }
}

// What lies in front of a tile.
struct TilePre {
  uint64_t kept, hdr;
  bool in_hdr;
  uint32_t own_hdr;  // header starts inside the tile
};
__device__ __forceinline__ TilePre tile_prefix(const SuperPre* super_pre, const uint4* tile_pre, uint64_t tile) {
  const SuperPre s = super_pre[tile / kTilesPerSuper];
  const uint4 p = tile_pre[tile];
  const FastaSum t = unpack_sum(p);
  const bool in = s.state != 0;
  return TilePre{s.kept + fa_kept_total(t, in), s.hdr + t.n_hdr, fa_state_out(t, in), p.x >> 2};
}

// Pass two: a wave per tile that holds a header start or begins inside a header line; every other tile costs its 16-byte entry.
__global__ __launch_bounds__(256) void fasta_record_kernel(const uint8_t* raw, uint64_t n, uint64_t n_tiles, const SuperPre* super_pre,
                                                           const uint4* tile_pre, uint64_t n_rec, uint64_t* hs_pos, uint64_t* kept_at,
                                                           uint64_t* hdr_end) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t tile = wave; tile < n_tiles; tile += n_waves) {
    const TilePre P = tile_prefix(super_pre, tile_pre, tile);
    if (!P.in_hdr && P.own_hdr == 0) continue;  // (the same in every lane)
    const uint64_t base = tile * kTile + 64ull * lane;
    uint4 v[4];
    load_lane(raw, n, base, v);
    uint64_t nl;
    uint32_t len;
    const FastaLane L = lane_masks(v, raw, n, tile * kTile, lane, &nl, &len);
    FastaSum excl, total;
    wave_scan(fa_summary(L), lane, &excl, &total);
    const bool in = fa_state_out(excl, P.in_hdr);
    const uint64_t kept_before = P.kept + fa_kept_total(excl, P.in_hdr), hdr_before = P.hdr + excl.n_hdr;
    const uint64_t hdr = fa_in_header(L.ls, L.hs, in), kept = L.cand & ~hdr;
    for (uint64_t m = L.hs; m; m &= m - 1) {
      const uint32_t i = (uint32_t)__ffsll((unsigned long long)m) - 1u;
      const uint64_t rec = hdr_before + fa_popc(L.hs & fa_below(i));
      if (rec < n_rec) {
        hs_pos[rec] = base + i;
        kept_at[rec] = kept_before + fa_popc(kept & fa_below(i));
      }
    }
    // a header line ends at its '\n', or with the input
    for (uint64_t m = nl & hdr; m; m &= m - 1) {
      const uint32_t i = (uint32_t)__ffsll((unsigned long long)m) - 1u;
      const uint64_t recs = hdr_before + fa_popc(L.hs & fa_below(i + 1));
      if (recs >= 1 && recs <= n_rec) hdr_end[recs - 1] = base + i;
    }
    if (len > 0 && base + len == n && ((hdr >> (len - 1)) & 1ull) && !((nl >> (len - 1)) & 1ull)) {
      const uint64_t recs = hdr_before + fa_popc(L.hs);
      if (recs >= 1 && recs <= n_rec) hdr_end[recs - 1] = n;
    }
  }
}

__device__ __forceinline__ uint64_t rec_len(const uint64_t* kept_at, uint64_t r, uint64_t n_rec, uint64_t total_kept) {
  return (r + 1 < n_rec ? kept_at[r + 1] : total_kept) - kept_at[r];
}
__device__ __forceinline__ uint64_t round64(uint64_t x) { return (x + 63ull) & ~63ull; }

// Inclusive Hillis-Steele over the 256 values of a workgroup; returns the exclusive value, *total the sum.
__device__ __forceinline__ uint64_t block_scan256(uint64_t v, unsigned long long* sh, uint64_t* total) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t o = 1; o < 256; o <<= 1) {
    const unsigned long long add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0ull;
    __syncthreads();
    sh[threadIdx.x] += add;
    __syncthreads();
  }
  *total = sh[255];
  return sh[threadIdx.x] - v;
}

// The layout bytes of every block of kRecBlock records.
__global__ __launch_bounds__(256) void fasta_rec_sum_kernel(const uint64_t* kept_at, uint64_t n_rec, uint64_t total_kept,
                                                            unsigned long long* block_sum) {
  __shared__ unsigned long long sh[256];
  const uint64_t r0 = (uint64_t)blockIdx.x * kRecBlock + (uint64_t)threadIdx.x * kRecPerThread;
  uint64_t mine = 0;
  for (uint32_t j = 0; j < kRecPerThread; ++j)
    if (r0 + j < n_rec) mine += round64(rec_len(kept_at, r0 + j, n_rec, total_kept));
  uint64_t total;
  (void)block_scan256(mine, sh, &total);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// Exclusive scan of the block sums in place, one workgroup; block_sum[n_blocks] = the layout's bytes.
__global__ __launch_bounds__(1024) void fasta_rec_top_kernel(unsigned long long* block_sum, uint64_t n_blocks) {
  __shared__ unsigned long long sums[1024];
  const uint64_t per = (n_blocks + 1023) / 1024;
  const uint64_t lo = min((uint64_t)threadIdx.x * per, n_blocks), hi = min(lo + per, n_blocks);
  unsigned long long mine = 0;
  for (uint64_t i = lo; i < hi; ++i) mine += block_sum[i];
  sums[threadIdx.x] = mine;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {
    const unsigned long long add = threadIdx.x >= o ? sums[threadIdx.x - o] : 0ull;
    __syncthreads();
    sums[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned long long run = sums[threadIdx.x] - mine;
  for (uint64_t i = lo; i < hi; ++i) {
    const unsigned long long c = block_sum[i];
    block_sum[i] = run;
    run += c;
  }
  if (threadIdx.x == 1023) block_sum[n_blocks] = sums[1023];
}

// The record table, and the zero pad behind every sequence (up to the next multiple of 64).
__global__ __launch_bounds__(256) void fasta_rec_write_kernel(const uint8_t* raw, uint64_t n, const uint64_t* hs_pos, const uint64_t* kept_at,
                                                              const uint64_t* hdr_end, uint64_t n_rec, uint64_t total_kept,
                                                              const unsigned long long* block_off, sassy_hip_FastaRecord* rec,
                                                              uint8_t* text, uint64_t layout_bytes) {
  __shared__ unsigned long long sh[256];
  const uint64_t r0 = (uint64_t)blockIdx.x * kRecBlock + (uint64_t)threadIdx.x * kRecPerThread;
  uint64_t lens[kRecPerThread], mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kRecPerThread; ++j) {
    lens[j] = r0 + j < n_rec ? rec_len(kept_at, r0 + j, n_rec, total_kept) : 0;
    mine += round64(lens[j]);
  }
  uint64_t total;
  uint64_t at = block_off[blockIdx.x] + block_scan256(mine, sh, &total);
#pragma unroll
  for (uint32_t j = 0; j < kRecPerThread; ++j) {
    if (r0 + j >= n_rec) break;
    const uint64_t hs = hs_pos[r0 + j], he = hdr_end[r0 + j];
    sassy_hip_FastaRecord R;
    R.id_start = hs + 1;
    R.id_len = 0;
    if (he > hs && he <= n) R.id_len = he - hs - 1 - (raw[he - 1] == 0x0D ? 1u : 0u);  // (byte hs is '>': he - 1 == hs strips nothing)
    R.seq_start = at;
    R.seq_len = lens[j];
    rec[r0 + j] = R;
    const uint64_t end = at + round64(lens[j]);
    if (end <= layout_bytes)
      for (uint64_t p = at + lens[j]; p < end; ++p) text[p] = 0;
    at = end;
  }
}

constexpr uint32_t kDumpByte = kTile + 31;  // (an image ends at 15 + 4096 at the latest)
// the four bytes of w whose bits in keep4 are set, to image[*at ...]
__device__ __forceinline__ void put4(uint8_t* image, uint32_t w, uint32_t keep4, uint32_t* at) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint32_t keep = (keep4 >> b) & 1u;
    image[keep ? *at : kDumpByte] = (uint8_t)(w >> (8 * b));
    *at += keep;
  }
}

// Pass three: a workgroup of one wave per tile in turn.
__global__ __launch_bounds__(64) void fasta_compact_kernel(const uint8_t* raw, uint64_t n, uint64_t n_tiles, const SuperPre* super_pre,
                                                           const uint4* tile_pre, const uint64_t* kept_at, const sassy_hip_FastaRecord* rec,
                                                           uint64_t n_rec, uint8_t* text, uint64_t layout_bytes) {
  __shared__ __attribute__((aligned(16))) uint8_t s_out[kTile + 32];  // the tile's kept bytes in order; the last byte takes what is dropped
  __shared__ uint16_t s_seg[kTile / 2];                               // a tile's header starts as ranks among its kept bytes
  const uint32_t lane = threadIdx.x;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const TilePre P = tile_prefix(super_pre, tile_pre, tile);
    uint4 v[4];
    load_lane(raw, n, tile * kTile + 64ull * lane, v);
    uint64_t nl;
    uint32_t len;
    const FastaLane L = lane_masks(v, raw, n, tile * kTile, lane, &nl, &len);
    FastaSum excl, total;
    wave_scan(fa_summary(L), lane, &excl, &total);
    const uint32_t kt = fa_kept_total(total, P.in_hdr);  // kept bytes of the tile
    if (kt == 0) continue;                               // (the same in every lane; no barrier skipped by a part of the wave)
    const bool in = fa_state_out(excl, P.in_hdr);
    const uint64_t kept = fa_kept(L, in);
    const uint32_t my_off = fa_kept_total(excl, P.in_hdr);  // kept bytes of the tile in front of this lane
    // a tile without a header start is one run of one record: where it begins; the LDS image is shifted so that 16-byte
    // pieces of it are 16-byte pieces of the text
    const bool one_run = P.own_hdr == 0;
    uint64_t d0 = 0;
    bool run_ok = false;
    if (one_run && P.hdr >= 1 && P.hdr <= n_rec) {
      const uint64_t r = P.hdr - 1;
      d0 = rec[r].seq_start + (P.kept - kept_at[r]);
      run_ok = d0 + kt <= layout_bytes;
    }
    const uint32_t shift = one_run ? (uint32_t)(d0 & 15ull) : 0u;
    // every lane puts its own kept bytes, straight from its registers, at their ranks in the tile's image; a dropped byte goes
    // to the spare byte behind the image, so that no store is predicated
    uint32_t at = shift + my_off;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      put4(s_out, v[j].x, (uint32_t)(kept >> (16 * j)), &at);
      put4(s_out, v[j].y, (uint32_t)(kept >> (16 * j + 4)), &at);
      put4(s_out, v[j].z, (uint32_t)(kept >> (16 * j + 8)), &at);
      put4(s_out, v[j].w, (uint32_t)(kept >> (16 * j + 12)), &at);
    }
    __syncthreads();
    if (one_run) {
      if (run_ok) {
        const uint64_t g0 = d0 - shift;  // a multiple of 16
        const uint32_t end = shift + kt;
        for (uint32_t c = lane; c < (end + 15u) / 16u; c += 64u) {
          const uint32_t lo = 16u * c, hi = lo + 16u;
          if (lo >= shift && hi <= end) {
            *reinterpret_cast<uint4*>(text + g0 + lo) = *reinterpret_cast<const uint4*>(s_out + lo);
          } else {
            for (uint32_t b = max(lo, shift); b < min(hi, end); ++b) text[g0 + b] = s_out[b];
          }
        }
      }
    } else {
      for (uint64_t m = L.hs; m; m &= m - 1) {
        const uint32_t i = (uint32_t)__ffsll((unsigned long long)m) - 1u;
        const uint32_t q = excl.n_hdr + fa_popc(L.hs & fa_below(i));
        if (q < kTile / 2) s_seg[q] = (uint16_t)(my_off + fa_popc(kept & fa_below(i)));
      }
      __syncthreads();
      const uint32_t n_seg = min(P.own_hdr, kTile / 2);
      for (uint32_t o = lane; o < kt; o += 64u) {
        uint32_t lo = 0, hi = n_seg;  // how many of the tile's header starts lie in front of kept byte o
        while (lo < hi) {
          const uint32_t mid = (lo + hi) / 2;
          if (s_seg[mid] <= o) lo = mid + 1;
          else hi = mid;
        }
        const uint64_t recs = P.hdr + lo;
        if (recs == 0 || recs > n_rec) continue;
        const uint64_t dst = rec[recs - 1].seq_start + (P.kept + o - kept_at[recs - 1]);
        if (dst < layout_bytes) text[dst] = s_out[o];
      }
    }
    __syncthreads();  // the next tile reuses the images
  }
}

// device memory of one call
struct Temps {
  std::vector<void*> p;
  ~Temps() {
    for (void* x : p) (void)hipFree(x);
  }
  template <typename T>
  int get(T** out, uint64_t count) {
    void* x = nullptr;
    const hipError_t e = hipMalloc(&x, std::max<uint64_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(SASSY_HIP_ENOMEM, "fasta_unwrap: out of device memory (" + std::to_string(count * sizeof(T)) + " bytes)");
    }
    p.push_back(x);
    *out = static_cast<T*>(x);
    return 0;
  }
};

int unwrap_on_device(const uint8_t* d_raw, uint64_t n, hipStream_t st, sassy_hip_Fasta* F) {
  const uint64_t n_tiles = (n + kTile - 1) / kTile, n_super = (n + kSuper - 1) / kSuper;
  Temps T;
  uint4 *tile_pre = nullptr, *super_sum = nullptr;
  SuperPre* super_pre = nullptr;
  if (int rc = T.get(&tile_pre, n_tiles)) return rc;
  if (int rc = T.get(&super_sum, n_super)) return rc;
  if (int rc = T.get(&super_pre, n_super + 1)) return rc;
  hipLaunchKernelGGL(fasta_count_kernel, dim3((uint32_t)n_super), dim3(256), 0, st, d_raw, n, n_tiles, tile_pre, super_sum);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fasta_scan_kernel, dim3(1), dim3(1024), 0, st, (const uint4*)super_sum, n_super, super_pre);
  HIP_TRY(hipGetLastError());
  SuperPre all{};
  HIP_TRY(hipMemcpyAsync(&all, super_pre + n_super, sizeof(all), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint64_t n_rec = all.hdr, total_kept = all.kept;
  if (n_rec > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "fasta_unwrap: " + std::to_string(n_rec) + " records, more than 2^32 - 1");
  if (n_rec == 0) return fail(SASSY_HIP_EINVAL, "fasta_unwrap: the input holds no record");  // (byte 0 is '>': cannot happen)

  const uint64_t n_blocks = (n_rec + kRecBlock - 1) / kRecBlock;
  uint64_t *hs_pos = nullptr, *kept_at = nullptr, *hdr_end = nullptr;
  unsigned long long* block_sum = nullptr;
  sassy_hip_FastaRecord* d_rec = nullptr;
  if (int rc = T.get(&hs_pos, n_rec)) return rc;
  if (int rc = T.get(&kept_at, n_rec)) return rc;
  if (int rc = T.get(&hdr_end, n_rec)) return rc;
  if (int rc = T.get(&block_sum, n_blocks + 1)) return rc;
  if (int rc = T.get(&d_rec, n_rec)) return rc;
  const uint32_t rec_grid = (uint32_t)std::min<uint64_t>((n_tiles + 3) / 4, 1u << 20);
  hipLaunchKernelGGL(fasta_record_kernel, dim3(rec_grid), dim3(256), 0, st, d_raw, n, n_tiles, (const SuperPre*)super_pre,
                     (const uint4*)tile_pre, n_rec, hs_pos, kept_at, hdr_end);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fasta_rec_sum_kernel, dim3((uint32_t)n_blocks), dim3(256), 0, st, (const uint64_t*)kept_at, n_rec, total_kept, block_sum);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fasta_rec_top_kernel, dim3(1), dim3(1024), 0, st, block_sum, n_blocks);
  HIP_TRY(hipGetLastError());
  unsigned long long layout = 0;
  HIP_TRY(hipMemcpyAsync(&layout, block_sum + n_blocks, sizeof(layout), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  F->text_bytes = layout + 64;
  if (hipMalloc(reinterpret_cast<void**>(&F->d_text), F->text_bytes) != hipSuccess) {
    (void)hipGetLastError();
    F->d_text = nullptr;
    return fail(SASSY_HIP_ENOMEM, "fasta_unwrap: out of device memory (" + std::to_string(F->text_bytes) + " bytes of text)");
  }
  HIP_TRY(hipMemsetAsync(F->d_text + layout, 0, 64, st));
  hipLaunchKernelGGL(fasta_rec_write_kernel, dim3((uint32_t)n_blocks), dim3(256), 0, st, d_raw, n, (const uint64_t*)hs_pos, (const uint64_t*)kept_at,
                     (const uint64_t*)hdr_end, n_rec, total_kept, (const unsigned long long*)block_sum, d_rec, F->d_text, (uint64_t)layout);
  HIP_TRY(hipGetLastError());
  const uint32_t grid = (uint32_t)std::min<uint64_t>(n_tiles, 256u * 16u);
  hipLaunchKernelGGL(fasta_compact_kernel, dim3(grid), dim3(64), 0, st, d_raw, n, n_tiles, (const SuperPre*)super_pre, (const uint4*)tile_pre,
                     (const uint64_t*)kept_at, (const sassy_hip_FastaRecord*)d_rec, n_rec, F->d_text, (uint64_t)layout);
  HIP_TRY(hipGetLastError());
  F->records.resize(n_rec);
  HIP_TRY(hipMemcpyAsync(F->records.data(), d_rec, n_rec * sizeof(sassy_hip_FastaRecord), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

}  // namespace

}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_fasta_unwrap(const void* raw, uint64_t n, uint32_t flags, void* hip_stream, sassy_hip_Fasta** out) {
  if (out) *out = nullptr;
  if (!out || (!raw && n)) return fail(SASSY_HIP_EINVAL, "null argument");
  if (flags & ~SASSY_HIP_TEXT_ON_DEVICE) return fail(SASSY_HIP_EINVAL, "fasta_unwrap takes SASSY_HIP_TEXT_ON_DEVICE only");
  const bool on_device = (flags & SASSY_HIP_TEXT_ON_DEVICE) != 0;
  if (on_device && ((uintptr_t)raw & 15) != 0) return fail(SASSY_HIP_EINVAL, "device pointer must be 16-byte aligned");
  if (n && !on_device && static_cast<const uint8_t*>(raw)[0] != '>') return fail(SASSY_HIP_EINVAL, "fasta_unwrap: the first byte is not '>'");
  if ((n + kSuper - 1) / kSuper > kMaxSuper)
    return fail(SASSY_HIP_EUNSUPPORTED, "fasta_unwrap: input too long for the tile index (more than 2^31 - 1 super-tiles of 64 KiB)");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    return fail(SASSY_HIP_ENODEVICE, "no usable HIP device (libsassy_hip has no CPU fallback; the FASTA unwrap runs on gfx950 only)");
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  std::unique_ptr<sassy_hip_Fasta> F(new sassy_hip_Fasta);
  struct Drop {
    std::unique_ptr<sassy_hip_Fasta>& f;
    ~Drop() {
      if (f && f->d_text) (void)hipFree(f->d_text);
    }
  } drop{F};
  HIP_TRY(hipGetDevice(&F->device));
  if (n == 0) {  // no record: the 64 spare bytes
    F->text_bytes = 64;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&F->d_text), 64));
    HIP_TRY(hipMemsetAsync(F->d_text, 0, 64, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out = F.release();
    return 0;
  }
  const uint8_t* d_raw = static_cast<const uint8_t*>(raw);
  uint8_t* d_up = nullptr;
  if (on_device) {
    uint8_t first = 0;
    HIP_TRY(hipMemcpyAsync(&first, d_raw, 1, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (first != '>') return fail(SASSY_HIP_EINVAL, "fasta_unwrap: the first byte is not '>'");
  } else {
    if (hipMalloc(reinterpret_cast<void**>(&d_up), n + 64) != hipSuccess) {
      (void)hipGetLastError();
      return fail(SASSY_HIP_ENOMEM, "fasta_unwrap: out of device memory (" + std::to_string(n + 64) + " bytes of input)");
    }
    const hipError_t e = hipMemcpyAsync(d_up, raw, n, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
      (void)hipFree(d_up);
      return hip_fail(e, "hipMemcpyAsync (fasta input)");
    }
    d_raw = d_up;
  }
  const int rc = unwrap_on_device(d_raw, n, st, F.get());
  if (d_up) {
    if (rc != 0) (void)hipStreamSynchronize(st);
    (void)hipFree(d_up);
  }
  if (rc != 0) return rc;
  *out = F.release();
  return 0;
}

uint64_t sassy_hip_fasta_n_records(const sassy_hip_Fasta* f) { return f ? f->records.size() : 0; }
const sassy_hip_FastaRecord* sassy_hip_fasta_records(const sassy_hip_Fasta* f) { return f && !f->records.empty() ? f->records.data() : nullptr; }
void* sassy_hip_fasta_text(const sassy_hip_Fasta* f) { return f ? f->d_text : nullptr; }
uint64_t sassy_hip_fasta_text_bytes(const sassy_hip_Fasta* f) { return f ? f->text_bytes : 0; }
void sassy_hip_fasta_free(sassy_hip_Fasta* f) {
  if (!f) return;
  if (f->d_text) (void)hipFree(f->d_text);
  delete f;
}

}  // extern "C"
