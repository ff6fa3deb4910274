// fastq_reads.hip -- a chunk of strict four-line FASTQ, raw bytes in, a read batch out that the Hamming batch kernels scan as
// it lies: records found and checked, every read's sequence laid out from a multiple of 64 bytes on with rem[] per block,
// all on the device (sassy_hip_fastq_parse), and the three Hamming batch calls over such a handle (sassy_hip_*_reads).
//
// The definition and the bit arithmetic are in fastq_step.h.  Geometry as line_index.hip and fasta_unwrap.hip: a tile = 4 KiB
// = what one wavefront holds in registers, 64 consecutive bytes per lane, 16-byte loads; a super-tile = 16 tiles = what one
// workgroup of the count pass reads.  Launches:
//   fastq_count_kernel   reads the raw bytes once; per tile the line starts in front of it INSIDE its super-tile, per
//                        super-tile its own line starts (32-bit)
//   fastq_scan_kernel    one workgroup: the exclusive scan of the super-tile counts, 64-bit; entry n_super = L  -> host
//   fastq_lines_kernel   reads the raw bytes again: every line start goes to line_start[line] (row line >> 2, column line & 3
//                        of its record), every stripped '\r' marks its line, a class 0 start without '@' or a class 2 start
//                        without '+' takes part in one atomicMin over the line numbers
//   fastq_rec_sum_kernel, fastq_rec_top_kernel   the lengths from consecutive line starts; the exclusive scan of the sequence
//                        lengths rounded up to 64 in blocks of 1024 records and one workgroup over the block sums
//   fastq_rec_write_kernel  the record table, starts[] and lens[] of the batch, the longest read; the layout's size  -> host
//   fastq_copy_kernel    a lane per 64-byte block of the OUTPUT: its read by ham_text_of, its bytes from the unaligned source
//                        with 16-byte loads and stores, zeros behind the read's end and in the 64 spare bytes, rem[block].
//                        Under SASSY_HIP_KEEP_QUALITY it runs once more, over line 4t + 3, into the handle's quality buffer
// Two host waits size what cannot be sized before: the line table (L) and the text (layout bytes).
// The record kernels take their lengths from a source: the lines of a file (the parse), the overlap records of a batch of
// pairs (reads_layout_merged, for merge_pairs.hip), the trim records of a batch or a table of window lengths
// (reads_layout_trimmed, reads_layout_windows, for trim_reads.hip), so the layout rule and its two-level scan have one owner.
#include "host_internal.h"
#include "fastq_step.h"
#include "hamming_step.h"
#include "merge_step.h"

// (struct sassy_hip_Reads: host_internal.h -- reads_relayout.hip reads it too)

namespace sassy_hip {

namespace {

constexpr uint32_t kTile = kFqTileBytes;
constexpr uint32_t kTilesPerSuper = 16;
constexpr uint64_t kSuper = (uint64_t)kTile * kTilesPerSuper;
constexpr uint64_t kMaxSuper = 0x7FFFFFFFull;  // a grid's width; DESIGN 10
constexpr uint32_t kRecPerThread = 4, kRecBlock = 256 * kRecPerThread;
constexpr unsigned long long kNoBadLine = ~0ull;
static_assert(kTile == 64 * kFqLaneBytes, "a tile is 64 lanes x 64 bytes");

// What the record kernels leave for the host, one readback.
struct FastqTotals {
  unsigned long long bad_line;  // the smallest line that lacks its marker
  unsigned long long layout;    // bytes of the layout
  unsigned long long longest;   // the longest sequence
  unsigned long long bad_qual;  // the smallest record whose quality is not as long as its sequence (looked at on request)
  unsigned long long filled;    // records the source counts (merged pairs, reads with an adapter), for the sources that ask for it
};

// The lane's 64 bytes of a tile as words.  raw is 16-byte aligned and readable up to the next multiple of 64 behind n, so a
// 16-byte load that starts in front of n is legal.
__device__ __forceinline__ void load_lane(const uint8_t* raw, uint64_t n, uint64_t base, uint32_t (&w)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (base + 16u * j < n) v = *reinterpret_cast<const uint4*>(raw + base + 16u * j);
    w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
  }
}

// The lane's masks; every lane of the wavefront calls this (shuffles).
__device__ __forceinline__ FastqLane lane_masks(const uint32_t (&w)[16], const uint8_t* raw, uint64_t n, uint64_t tile_base, uint32_t lane,
                                                uint32_t* len_out) {
  const uint64_t base = tile_base + 64ull * lane;
  const uint32_t len = base >= n ? 0u : (uint32_t)min((uint64_t)64, n - base);
  const uint64_t valid = fq_below(len);
  const uint64_t nl = fq_eq_bits64(w, 0x0A) & valid, cr = fq_eq_bits64(w, 0x0D) & valid;
  const uint32_t last_nl = (uint32_t)(nl >> 63), first_end = len == 0 ? 1u : (uint32_t)(nl & 1ull);
  uint32_t prev = __shfl_up(last_nl, 1, 64), next = __shfl_down(first_end, 1, 64);
  if (lane == 0) prev = tile_base == 0 ? 1u : (raw[tile_base - 1] == 0x0A ? 1u : 0u);
  if (lane == 63) {
    const uint64_t q = tile_base + kTile;
    next = q >= n ? 1u : (raw[q] == 0x0A ? 1u : 0u);
  }
  *len_out = len;
  return fq_lane(nl, cr, len, prev != 0, next != 0);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor(v, o, 64);
  return v;
}
// the sum of the lanes in front of this one
__device__ __forceinline__ uint32_t wave_excl(uint32_t mine, uint32_t lane) {
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if ((int)lane >= o) incl += up;
  }
  return incl - mine;
}

// Pass one: a workgroup per super-tile, a wave per four of its tiles.
__global__ __launch_bounds__(256) void fastq_count_kernel(const uint8_t* raw, uint64_t n, uint64_t n_tiles, uint32_t* tile_pre, uint32_t* super_sum) {
  __shared__ uint32_t sums[kTilesPerSuper];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t tile0 = (uint64_t)blockIdx.x * kTilesPerSuper;
  for (uint32_t i = 0; i < kTilesPerSuper / 4; ++i) {
    const uint32_t t = wave * (kTilesPerSuper / 4) + i;
    uint32_t s = 0;
    if (tile0 + t < n_tiles) {  // (the same in every lane of the wave)
      uint32_t w[16];
      load_lane(raw, n, (tile0 + t) * kTile + 64ull * lane, w);
      uint32_t len;
      s = wave_sum(fq_count(lane_masks(w, raw, n, (tile0 + t) * kTile, lane, &len)));
    }
    if (lane == 0) sums[t] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (uint32_t t = 0; t < kTilesPerSuper; ++t) {
      if (tile0 + t < n_tiles) tile_pre[tile0 + t] = run;
      run += sums[t];
    }
    super_sum[blockIdx.x] = run;
  }
}

// The exclusive scan of the super-tile counts: one workgroup, a contiguous run of entries per thread.  super_pre has
// n_super + 1 entries, the last one the number of lines.
__global__ __launch_bounds__(1024) void fastq_scan_kernel(const uint32_t* super_sum, uint64_t n_super, unsigned long long* super_pre) {
  __shared__ unsigned long long sums[1024];
  const uint64_t per = (n_super + 1023) / 1024;
  const uint64_t lo = min((uint64_t)threadIdx.x * per, n_super), hi = min(lo + per, n_super);
  unsigned long long mine = 0;
  for (uint64_t i = lo; i < hi; ++i) mine += super_sum[i];
  sums[threadIdx.x] = mine;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {  // Hillis-Steele, inclusive
    const unsigned long long add = threadIdx.x >= o ? sums[threadIdx.x - o] : 0ull;
    __syncthreads();
    sums[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned long long run = sums[threadIdx.x] - mine;
  for (uint64_t i = lo; i < hi; ++i) {
    super_pre[i] = run;
    run += super_sum[i];
  }
  if (threadIdx.x == 1023) super_pre[n_super] = sums[1023];
}

// Pass two: a wave per tile in turn.  line_cr is zero on entry.
__global__ __launch_bounds__(256) void fastq_lines_kernel(const uint8_t* raw, uint64_t n, uint64_t n_tiles, const unsigned long long* super_pre,
                                                          const uint32_t* tile_pre, uint64_t n_lines, uint64_t* line_start, uint8_t* line_cr,
                                                          FastqTotals* totals) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t tile = wave; tile < n_tiles; tile += n_waves) {
    const uint64_t base = tile * kTile + 64ull * lane;
    uint32_t w[16];
    load_lane(raw, n, base, w);
    uint32_t len;
    const FastqLane L = lane_masks(w, raw, n, tile * kTile, lane, &len);
    const uint64_t front = fq_front(super_pre[tile / kTilesPerSuper], tile_pre[tile]) + wave_excl(fq_count(L), lane);
    const uint64_t at = fq_eq_bits64(w, '@'), plus = fq_eq_bits64(w, '+');
    unsigned long long bad = kNoBadLine;
    for (uint64_t m = L.ls; m; m &= m - 1) {
      const uint32_t i = (uint32_t)__ffsll((unsigned long long)m) - 1u;
      const uint64_t line = fq_line_of_start(L, front, i);
      if (line < n_lines) line_start[line] = base + i;
      const uint32_t cls = fq_class(line);
      const bool ok = cls == 0 ? ((at >> i) & 1ull) != 0 : cls == 2 ? ((plus >> i) & 1ull) != 0 : true;
      if (!ok && line < bad) bad = line;
    }
    for (uint64_t m = L.strip; m; m &= m - 1) {
      const uint32_t i = (uint32_t)__ffsll((unsigned long long)m) - 1u;
      const uint64_t line = fq_line_of_byte(L, front, i);
      if (line < n_lines) line_cr[line] = 1;
    }
    if (bad != kNoBadLine) atomicMin(&totals->bad_line, bad);
  }
}

__device__ __forceinline__ uint64_t line_len(const uint64_t* line_start, const uint8_t* line_cr, uint64_t line, uint64_t n_lines, uint64_t virt) {
  const uint64_t next = line + 1 < n_lines ? line_start[line + 1] : virt;
  return fq_line_len(line_start[line], next, line_cr[line] != 0);
}

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

// Where the record kernels take the lengths from, and what a record says besides.  The lines of a file ...
struct LineSource {
  const uint64_t* line_start;
  const uint8_t* line_cr;
  uint64_t n_rec, virt;
  bool check_qual;  // report the smallest record with qual_len != seq_len
  static constexpr bool kCountFilled = false;
  __device__ __forceinline__ uint64_t len(uint64_t r) const { return line_len(line_start, line_cr, 4 * r + 1, 4 * n_rec, virt); }
  __device__ __forceinline__ sassy_hip_ReadRecord record(uint64_t r, uint64_t at, uint64_t seq_len) const {
    sassy_hip_ReadRecord R;
    R.id_start = line_start[4 * r] + 1;
    R.id_len = line_len(line_start, line_cr, 4 * r, 4 * n_rec, virt) - 1;  // (the line begins with '@': checked before the table is used)
    R.seq_start = at;
    R.seq_len = seq_len;
    R.qual_start = line_start[4 * r + 3];
    R.qual_len = line_len(line_start, line_cr, 4 * r + 3, 4 * n_rec, virt);
    return R;
  }
};
// ... or the overlap records of a batch of pairs: read r is the merged read of pair r (merge_step.h), empty where the pair
// has no accepted overlap.  No ids; the quality lies in the handle's own buffer, where the sequence lies in the text.
struct MergedSource {
  const sassy_hip_ReadOverlap* rec;
  const uint64_t *len1, *len2;
  static constexpr bool check_qual = false;
  static constexpr bool kCountFilled = true;
  __device__ __forceinline__ uint64_t len(uint64_t r) const {
    const sassy_hip_ReadOverlap o = rec[r];
    // (a record with an accepted offset comes from reads of at most kOvlMaxLen bytes; the clamp keeps a length sane whatever it holds)
    const uint32_t la = (uint32_t)min(len1[r], (uint64_t)kOvlMaxLen), lb = (uint32_t)min(len2[r], (uint64_t)kOvlMaxLen);
    return min(mrg_length(la, lb, OvlBest{o.offset, o.overlap, o.mismatches, o.n_accepted}), 2u * kOvlMaxLen);
  }
  __device__ __forceinline__ bool counted(uint64_t, uint64_t seq_len) const { return seq_len != 0; }  // the merged pairs
  __device__ __forceinline__ sassy_hip_ReadRecord record(uint64_t, uint64_t at, uint64_t seq_len) const {
    return sassy_hip_ReadRecord{0, 0, at, seq_len, at, seq_len};
  }
};
// ... or the trim records of a batch (trim_step.h): read r is what the trim leaves of read r, empty where it was dropped.  No
// ids; a quality, where the handle keeps one, lies where the sequence lies.
struct TrimSource {
  const sassy_hip_ReadTrim* rec;
  bool keep_quality;
  static constexpr bool check_qual = false;
  static constexpr bool kCountFilled = true;
  __device__ __forceinline__ uint64_t len(uint64_t r) const { return min(rec[r].length, (uint32_t)kOvlMaxLen); }  // (a cut lies inside its read)
  __device__ __forceinline__ bool counted(uint64_t r, uint64_t) const { return rec[r].adapter >= 0; }  // the reads with an adapter found
  __device__ __forceinline__ sassy_hip_ReadRecord record(uint64_t, uint64_t at, uint64_t seq_len) const {
    return sassy_hip_ReadRecord{0, 0, at, seq_len, keep_quality ? at : 0, keep_quality ? seq_len : 0};
  }
};
// ... or a table of window lengths (sassy_hip_reads_slice), checked against the reads by the host
struct WindowSource {
  const uint64_t* lens;
  bool keep_quality;
  static constexpr bool check_qual = false;
  static constexpr bool kCountFilled = false;
  __device__ __forceinline__ uint64_t len(uint64_t r) const { return lens[r]; }
  __device__ __forceinline__ sassy_hip_ReadRecord record(uint64_t, uint64_t at, uint64_t seq_len) const {
    return sassy_hip_ReadRecord{0, 0, at, seq_len, keep_quality ? at : 0, keep_quality ? seq_len : 0};
  }
};

// The layout bytes of every block of kRecBlock records.
template <typename Src>
__global__ __launch_bounds__(256) void fastq_rec_sum_kernel(Src S, uint64_t n_rec, unsigned long long* block_sum) {
  __shared__ unsigned long long sh[256];
  const uint64_t r0 = (uint64_t)blockIdx.x * kRecBlock + (uint64_t)threadIdx.x * kRecPerThread;
  uint64_t mine = 0;
  for (uint32_t j = 0; j < kRecPerThread; ++j)
    if (r0 + j < n_rec) mine += fq_round64(S.len(r0 + j));
  uint64_t total;
  (void)block_scan256(mine, sh, &total);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// Exclusive scan of the block sums in place, one workgroup; block_sum[n_blocks] = the layout's bytes, which go to the totals.
__global__ __launch_bounds__(1024) void fastq_rec_top_kernel(unsigned long long* block_sum, uint64_t n_blocks, FastqTotals* totals) {
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
  if (threadIdx.x == 1023) {
    block_sum[n_blocks] = sums[1023];
    totals->layout = sums[1023];
  }
}

// The record table, the batch's starts[] and lens[] (table: starts first), the longest read.
template <typename Src>
__global__ __launch_bounds__(256) void fastq_rec_write_kernel(Src S, uint64_t n_rec, const unsigned long long* block_off, sassy_hip_ReadRecord* rec,
                                                              uint64_t* table, FastqTotals* totals) {
  __shared__ unsigned long long sh[256];
  const uint64_t r0 = (uint64_t)blockIdx.x * kRecBlock + (uint64_t)threadIdx.x * kRecPerThread;
  uint64_t lens[kRecPerThread], mine = 0, longest = 0;
  uint32_t filled = 0;
#pragma unroll
  for (uint32_t j = 0; j < kRecPerThread; ++j) {
    lens[j] = r0 + j < n_rec ? S.len(r0 + j) : 0;
    mine += fq_round64(lens[j]);
    longest = max(longest, lens[j]);
    if constexpr (Src::kCountFilled) filled += r0 + j < n_rec && S.counted(r0 + j, lens[j]);
  }
  uint64_t total;
  uint64_t at = block_off[blockIdx.x] + block_scan256(mine, sh, &total);
  unsigned long long bad = kNoBadLine;
#pragma unroll
  for (uint32_t j = 0; j < kRecPerThread; ++j) {
    const uint64_t r = r0 + j;
    if (r >= n_rec) break;
    const sassy_hip_ReadRecord R = S.record(r, at, lens[j]);
    if (S.check_qual && R.qual_len != R.seq_len && r < bad) bad = r;
    rec[r] = R;
    table[r] = at;
    table[n_rec + r] = lens[j];
    at += fq_round64(lens[j]);
  }
  if (bad != kNoBadLine) atomicMin(&totals->bad_qual, bad);  // (well-formed input never comes here)
  // one atomic per wavefront at the most, and none once the maximum stands: reads of one length would otherwise queue
  // every thread of the grid on one address
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) longest = max(longest, (uint64_t)__shfl_xor((unsigned long long)longest, o, 64));
  if ((threadIdx.x & 63u) == 0 && longest > __hip_atomic_load(&totals->longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(&totals->longest, (unsigned long long)longest);
  if constexpr (Src::kCountFilled) {
    filled = wave_sum(filled);
    if ((threadIdx.x & 63u) == 0 && filled) atomicAdd(&totals->filled, (unsigned long long)filled);
  }
}

// Pass three: a lane per 64-byte block of the layout, and one more for the spare bytes behind it.  n_pad: up to where raw is
// readable (the next multiple of 64 behind n).  `line`: which line of a record is copied -- 1, the sequence, into the text, or
// 3, the quality, into a buffer of the same layout (rem: null then, it is the text's).
__global__ __launch_bounds__(256) void fastq_copy_kernel(const uint8_t* raw, uint64_t n_pad, const uint64_t* line_start, uint32_t line,
                                                         const uint64_t* table, uint32_t n_rec, uint64_t n_blocks, uint8_t* text, uint32_t* rem) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > n_blocks) return;
  uint32_t out[16];
  if (b == n_blocks) {
#pragma unroll
    for (int j = 0; j < 16; ++j) out[j] = 0u;
  } else {
    const uint32_t t = ham_text_of([&](uint32_t i) { return table[i]; }, n_rec, b * 64);
    const uint64_t start = table[t];
    const uint32_t left = ham_rem(b, start, table[(uint64_t)n_rec + t]);
    if (rem) rem[b] = left;
    const uint64_t src = line_start[4ull * t + line] + (b * 64 - start), a = src & ~15ull;
    uint32_t w[20];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (a + 16u * j < n_pad) v = *reinterpret_cast<const uint4*>(raw + a + 16u * j);
      w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
    }
    fq_shift_block(w, (uint32_t)(src & 15ull), min(left, 64u), out);
  }
  uint4* dst = reinterpret_cast<uint4*>(text + b * 64);
#pragma unroll
  for (int j = 0; j < 4; ++j) dst[j] = make_uint4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
}

// device memory of one call; who: the call's name, for its messages
struct Temps {
  const char* who;
  std::vector<void*> p;
  explicit Temps(const char* who_) : who(who_) {}
  ~Temps() {
    for (void* x : p) (void)hipFree(x);
  }
  template <typename T>
  int get(T** out, uint64_t count) {
    void* x = nullptr;
    const hipError_t e = hipMalloc(&x, std::max<uint64_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(SASSY_HIP_ENOMEM, std::string(who) + ": out of device memory (" + std::to_string(count * sizeof(T)) + " bytes)");
    }
    p.push_back(x);
    *out = static_cast<T*>(x);
    return 0;
  }
};

template <typename T>
int own(T** out, uint64_t count, const char* what, const char* who) {
  if (hipMalloc(reinterpret_cast<void**>(out), std::max<uint64_t>(count, 1) * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return fail(SASSY_HIP_ENOMEM, std::string(who) + ": out of device memory (" + std::to_string(count * sizeof(T)) + " bytes of " + what + ")");
  }
  return 0;
}

int malformed(uint64_t n_lines, uint64_t bad_line) {
  const FastqVerdict v = fq_verdict(n_lines, bad_line);
  const std::string rec = "fastq_parse: record " + std::to_string(v.record);
  if (v.rule == kFqNoAt) return fail(SASSY_HIP_EINVAL, rec + ": its first line does not begin with '@'");
  if (v.rule == kFqNoPlus) return fail(SASSY_HIP_EINVAL, rec + ": its third line does not begin with '+'");
  return fail(SASSY_HIP_EINVAL, rec + ": it has " + std::to_string(n_lines - 4 * v.record) + " of its four lines (strict four-line FASTQ)");
}

// The record kernels over a source of n_rec lengths: the handle's device table, the records on the device (*d_rec, T's) and the
// totals on the host.  d_totals is initialised by the caller; the one host wait of the layout is here.
template <typename Src>
int layout_records(const Src& S, uint64_t n_rec, hipStream_t st, Temps& T, sassy_hip_Reads* F, FastqTotals* d_totals, FastqTotals* tot,
                   sassy_hip_ReadRecord** d_rec) {
  const uint64_t n_blocks = (n_rec + kRecBlock - 1) / kRecBlock;
  unsigned long long* block_sum = nullptr;
  if (int rc = T.get(&block_sum, n_blocks + 1)) return rc;
  if (int rc = T.get(d_rec, n_rec)) return rc;
  if (int rc = own(&F->d_table, 2 * n_rec, "read table", T.who)) return rc;
  hipLaunchKernelGGL(fastq_rec_sum_kernel<Src>, dim3((uint32_t)n_blocks), dim3(256), 0, st, S, n_rec, block_sum);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fastq_rec_top_kernel, dim3(1), dim3(1024), 0, st, block_sum, n_blocks, d_totals);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fastq_rec_write_kernel<Src>, dim3((uint32_t)n_blocks), dim3(256), 0, st, S, n_rec, (const unsigned long long*)block_sum, *d_rec,
                     F->d_table, d_totals);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(tot, d_totals, sizeof(*tot), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}
// The buffers the totals size: the text, the block table and, on request, the quality buffer of the text's layout.  who: the
// call's name, here and below.
int layout_buffers(const FastqTotals& tot, bool keep_quality, sassy_hip_Reads* F, const char* who) {
  F->longest = tot.longest;
  F->text_bytes = tot.layout + 64;
  if (int rc = own(&F->d_text, F->text_bytes, "text", who)) return rc;
  if (keep_quality)
    if (int rc = own(&F->d_qual, F->text_bytes, "quality", who)) return rc;
  if (int rc = own(&F->d_rem, tot.layout / 64, "block table", who)) return rc;
  if (tot.layout / 64 + 1 + 255 > 0xFFFFFFFFull * 256ull) return fail(SASSY_HIP_EUNSUPPORTED, std::string(who) + ": the layout is too long for a grid");
  return 0;
}
// the record table's host copy; returns when it has landed.  lane: a searcher's, whose pinned buffers carry the copy as they
// carry every result's; the parse has no searcher and copies plainly
int take_records(const sassy_hip_ReadRecord* d_rec, uint64_t n_rec, hipStream_t st, ScanLane* lane, sassy_hip_Reads* F, const char* who) {
  F->records.reset(new (std::nothrow) sassy_hip_ReadRecord[n_rec]);
  if (!F->records) return fail(SASSY_HIP_ENOMEM, std::string(who) + ": out of host memory (" + std::to_string(n_rec) + " records)");
  F->n_records = n_rec;
  if (lane) return lane->download(F->records.get(), d_rec, n_rec * sizeof(sassy_hip_ReadRecord));
  HIP_TRY(hipMemcpyAsync(F->records.get(), d_rec, n_rec * sizeof(sassy_hip_ReadRecord), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

// last_is_nl: byte n - 1 is '\n'
int parse_on_device(const uint8_t* d_raw, uint64_t n, bool last_is_nl, bool keep_quality, hipStream_t st, sassy_hip_Reads* F) {
  const uint64_t n_tiles = (n + kTile - 1) / kTile, n_super = (n + kSuper - 1) / kSuper;
  Temps T("fastq_parse");
  uint32_t *tile_pre = nullptr, *super_sum = nullptr;
  unsigned long long* super_pre = nullptr;
  FastqTotals* d_totals = nullptr;
  if (int rc = T.get(&tile_pre, n_tiles)) return rc;
  if (int rc = T.get(&super_sum, n_super)) return rc;
  if (int rc = T.get(&super_pre, n_super + 1)) return rc;
  if (int rc = T.get(&d_totals, 1)) return rc;
  const FastqTotals zero{kNoBadLine, 0, 0, kNoBadLine, 0};
  HIP_TRY(hipMemcpyAsync(d_totals, &zero, sizeof(zero), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(fastq_count_kernel, dim3((uint32_t)n_super), dim3(256), 0, st, d_raw, n, n_tiles, tile_pre, super_sum);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fastq_scan_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)super_sum, n_super, super_pre);
  HIP_TRY(hipGetLastError());
  unsigned long long n_lines = 0;
  HIP_TRY(hipMemcpyAsync(&n_lines, super_pre + n_super, sizeof(n_lines), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (this wait also covers `zero`)
  const uint64_t n_rec = n_lines / 4;
  if (n_rec > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "fastq_parse: " + std::to_string(n_rec) + " records, more than 2^32 - 1");

  uint64_t* line_start = nullptr;
  uint8_t* line_cr = nullptr;
  if (int rc = T.get(&line_start, n_lines)) return rc;
  if (int rc = T.get(&line_cr, n_lines)) return rc;
  HIP_TRY(hipMemsetAsync(line_cr, 0, std::max<uint64_t>(n_lines, 1), st));
  const uint32_t line_grid = (uint32_t)std::min<uint64_t>((n_tiles + 3) / 4, 1u << 20);
  hipLaunchKernelGGL(fastq_lines_kernel, dim3(line_grid), dim3(256), 0, st, d_raw, n, n_tiles, (const unsigned long long*)super_pre,
                     (const uint32_t*)tile_pre, (uint64_t)n_lines, line_start, line_cr, d_totals);
  HIP_TRY(hipGetLastError());
  FastqTotals tot{};
  if (n_lines % 4) {  // the record kernels take whole records: the verdict needs the markers only
    HIP_TRY(hipMemcpyAsync(&tot, d_totals, sizeof(tot), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return malformed(n_lines, tot.bad_line);
  }

  sassy_hip_ReadRecord* d_rec = nullptr;
  const LineSource S{line_start, line_cr, n_rec, fq_virtual_start(n, last_is_nl), keep_quality};
  if (int rc = layout_records(S, n_rec, st, T, F, d_totals, &tot, &d_rec)) return rc;
  if (tot.bad_line != kNoBadLine) return malformed(n_lines, tot.bad_line);  // (the lengths of such an input mean nothing)
  if (tot.bad_qual != kNoBadLine)  // (looked at under SASSY_HIP_KEEP_QUALITY only, and behind every older verdict)
    return fail(SASSY_HIP_EINVAL, "fastq_parse: record " + std::to_string(tot.bad_qual) +
                                      ": its quality is not as long as its sequence (SASSY_HIP_KEEP_QUALITY keeps one quality byte per base)");

  if (int rc = layout_buffers(tot, keep_quality, F, T.who)) return rc;
  const uint64_t text_blocks = tot.layout / 64;
  const dim3 grid((uint32_t)((text_blocks + 1 + 255) / 256));
  hipLaunchKernelGGL(fastq_copy_kernel, grid, dim3(256), 0, st, d_raw, (n + 63) & ~63ull, (const uint64_t*)line_start, 1u,
                     (const uint64_t*)F->d_table, (uint32_t)n_rec, text_blocks, F->d_text, F->d_rem);
  HIP_TRY(hipGetLastError());
  if (keep_quality) {
    hipLaunchKernelGGL(fastq_copy_kernel, grid, dim3(256), 0, st, d_raw, (n + 63) & ~63ull, (const uint64_t*)line_start, 3u,
                       (const uint64_t*)F->d_table, (uint32_t)n_rec, text_blocks, F->d_qual, (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
  }
  return take_records(d_rec, n_rec, st, nullptr, F, T.who);
}

// ---- the batch calls over a handle ----
int reads_pointers(const sassy_SearcherType* s, bool have_out, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                   const sassy_hip_Reads* reads, const char* who) {
  if (!s || !have_out || !reads || (n_patterns && (!patterns || !pattern_lens)))
    return fail(SASSY_HIP_EINVAL, std::string("Pointers in ") + who + "() must not be null");
  return 0;
}
// the handle as the one batch the drivers scan, whole: text0 = 0
HamText reads_text(const sassy_hip_Reads* r) {
  HamText t;
  t.d_text = r->d_text; t.n = r->text_bytes - 64; t.longest = r->longest;
  t.rem = r->d_rem; t.starts = r->d_table; t.n_texts = (uint32_t)r->n_records; t.text0 = 0;
  return t;
}

}  // namespace

// For merge_pairs.hip: a new handle of n reads whose lengths are the merged lengths of the pairs behind d_rec (the overlap
// records of a call, on the device) and the two handles' length tables.  Leaves the table, the records and the longest read
// in F and its text, quality and block buffers allocated, for the caller's kernel to fill; *n_merged: the reads that are not
// empty.  n > 0.  lane: the searcher's, for its stream and its pinned buffers.
int reads_layout_merged(const sassy_hip_ReadOverlap* d_rec, const uint64_t* d_len1, const uint64_t* d_len2, uint64_t n, ScanLane* lane,
                        sassy_hip_Reads* F, uint64_t* n_merged) {
  hipStream_t st = lane->stream;
  Temps T("merge_pairs");
  FastqTotals* d_totals = nullptr;
  if (int rc = T.get(&d_totals, 1)) return rc;
  const FastqTotals zero{kNoBadLine, 0, 0, kNoBadLine, 0};
  HIP_TRY(hipMemcpyAsync(d_totals, &zero, sizeof(zero), hipMemcpyHostToDevice, st));
  FastqTotals tot{};
  sassy_hip_ReadRecord* d_records = nullptr;
  if (int rc = layout_records(MergedSource{d_rec, d_len1, d_len2}, n, st, T, F, d_totals, &tot, &d_records)) return rc;
  if (int rc = layout_buffers(tot, true, F, T.who)) return rc;
  *n_merged = tot.filled;
  return take_records(d_records, n, st, lane, F, T.who);
}


// For trim_reads.hip: a new handle of n reads whose lengths are the `length` of the trim records behind d_rec (on the device),
// with a quality buffer where asked for; *n_found: the reads whose record names an adapter.  As reads_layout_merged otherwise.
int reads_layout_trimmed(const sassy_hip_ReadTrim* d_rec, uint64_t n, bool keep_quality, ScanLane* lane, sassy_hip_Reads* F, uint64_t* n_found) {
  hipStream_t st = lane->stream;
  Temps T("trim_reads");
  FastqTotals* d_totals = nullptr;
  if (int rc = T.get(&d_totals, 1)) return rc;
  const FastqTotals zero{kNoBadLine, 0, 0, kNoBadLine, 0};
  HIP_TRY(hipMemcpyAsync(d_totals, &zero, sizeof(zero), hipMemcpyHostToDevice, st));
  FastqTotals tot{};
  sassy_hip_ReadRecord* d_records = nullptr;
  if (int rc = layout_records(TrimSource{d_rec, keep_quality}, n, st, T, F, d_totals, &tot, &d_records)) return rc;
  if (int rc = layout_buffers(tot, keep_quality, F, T.who)) return rc;
  *n_found = tot.filled;
  return take_records(d_records, n, st, lane, F, T.who);
}
// ... and one whose lengths are a table on the device (sassy_hip_reads_slice: no searcher, so a plain stream)
int reads_layout_windows(const uint64_t* d_lens, uint64_t n, bool keep_quality, hipStream_t st, sassy_hip_Reads* F) {
  Temps T("reads_slice");
  FastqTotals* d_totals = nullptr;
  if (int rc = T.get(&d_totals, 1)) return rc;
  const FastqTotals zero{kNoBadLine, 0, 0, kNoBadLine, 0};
  HIP_TRY(hipMemcpyAsync(d_totals, &zero, sizeof(zero), hipMemcpyHostToDevice, st));
  FastqTotals tot{};
  sassy_hip_ReadRecord* d_records = nullptr;
  if (int rc = layout_records(WindowSource{d_lens, keep_quality}, n, st, T, F, d_totals, &tot, &d_records)) return rc;
  if (int rc = layout_buffers(tot, keep_quality, F, T.who)) return rc;
  return take_records(d_records, n, st, nullptr, F, T.who);
}

}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_fastq_parse(const void* raw, uint64_t n, uint32_t flags, void* hip_stream, sassy_hip_Reads** out) {
  if (out) *out = nullptr;
  if (!out || (!raw && n)) return fail(SASSY_HIP_EINVAL, "null argument");
  if (flags & ~(SASSY_HIP_TEXT_ON_DEVICE | SASSY_HIP_KEEP_QUALITY))
    return fail(SASSY_HIP_EINVAL, "fastq_parse takes SASSY_HIP_TEXT_ON_DEVICE only, and SASSY_HIP_KEEP_QUALITY");
  const bool on_device = (flags & SASSY_HIP_TEXT_ON_DEVICE) != 0, keep_quality = (flags & SASSY_HIP_KEEP_QUALITY) != 0;
  if (on_device && ((uintptr_t)raw & 15) != 0) return fail(SASSY_HIP_EINVAL, "device pointer must be 16-byte aligned");
  if (n && !on_device && static_cast<const uint8_t*>(raw)[0] != '@') return fail(SASSY_HIP_EINVAL, "fastq_parse: the first byte is not '@'");
  if ((n + kSuper - 1) / kSuper > kMaxSuper)
    return fail(SASSY_HIP_EUNSUPPORTED, "fastq_parse: input too long for the tile index (more than 2^31 - 1 super-tiles of 64 KiB)");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    return fail(SASSY_HIP_ENODEVICE, "no usable HIP device (libsassy_hip has no CPU fallback; the FASTQ parse runs on gfx950 only)");
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  std::unique_ptr<sassy_hip_Reads> F(new sassy_hip_Reads);
  struct Drop {
    std::unique_ptr<sassy_hip_Reads>& f;
    ~Drop() {
      if (f) f->release();
    }
  } drop{F};
  HIP_TRY(hipGetDevice(&F->device));
  if (n == 0) {  // no record: the 64 spare bytes
    F->text_bytes = 64;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&F->d_text), 64));
    HIP_TRY(hipMemsetAsync(F->d_text, 0, 64, st));
    if (keep_quality) {
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&F->d_qual), 64));
      HIP_TRY(hipMemsetAsync(F->d_qual, 0, 64, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    *out = F.release();
    return 0;
  }
  const uint8_t* d_raw = static_cast<const uint8_t*>(raw);
  uint8_t* d_up = nullptr;
  uint8_t last = 0;
  if (on_device) {
    uint8_t first = 0;
    HIP_TRY(hipMemcpyAsync(&first, d_raw, 1, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last, d_raw + n - 1, 1, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (first != '@') return fail(SASSY_HIP_EINVAL, "fastq_parse: the first byte is not '@'");
  } else {
    last = static_cast<const uint8_t*>(raw)[n - 1];
    if (hipMalloc(reinterpret_cast<void**>(&d_up), n + 64) != hipSuccess) {
      (void)hipGetLastError();
      return fail(SASSY_HIP_ENOMEM, "fastq_parse: out of device memory (" + std::to_string(n + 64) + " bytes of input)");
    }
    const hipError_t e = hipMemcpyAsync(d_up, raw, n, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
      (void)hipFree(d_up);
      return hip_fail(e, "hipMemcpyAsync (fastq input)");
    }
    d_raw = d_up;
  }
  const int rc = parse_on_device(d_raw, n, last == 0x0A, keep_quality, st, F.get());
  if (d_up) {
    if (rc != 0) (void)hipStreamSynchronize(st);
    (void)hipFree(d_up);
  }
  if (rc != 0) return rc;
  *out = F.release();
  return 0;
}

uint64_t sassy_hip_reads_n(const sassy_hip_Reads* r) { return r ? r->n_records : 0; }
const sassy_hip_ReadRecord* sassy_hip_reads_records(const sassy_hip_Reads* r) { return r && r->n_records ? r->records.get() : nullptr; }
void* sassy_hip_reads_text(const sassy_hip_Reads* r) { return r ? r->d_text : nullptr; }
uint64_t sassy_hip_reads_text_bytes(const sassy_hip_Reads* r) { return r ? r->text_bytes : 0; }
uint64_t sassy_hip_reads_longest(const sassy_hip_Reads* r) { return r ? r->longest : 0; }
const uint32_t* sassy_hip_reads_rem(const sassy_hip_Reads* r) { return r ? r->d_rem : nullptr; }
const uint8_t* sassy_hip_reads_quality(const sassy_hip_Reads* r) { return r ? r->d_qual : nullptr; }
void sassy_hip_reads_free(sassy_hip_Reads* r) {
  if (!r) return;
  r->release();
  delete r;
}

int sassy_hip_search_hamming_reads(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                   const sassy_hip_Reads* reads, size_t k, uint32_t flags, sassy_hip_Result** out) {
  const char* who = "search_hamming_reads";
  if (out) *out = nullptr;
  if (int rc = reads_pointers(s, out != nullptr, patterns, pattern_lens, n_patterns, reads, who)) return rc;
  if (flags & ~(uint32_t)SASSY_HIP_WITHOUT_TRACE) return fail(SASSY_HIP_EINVAL, "search_hamming_reads takes SASSY_HIP_WITHOUT_TRACE only");
  if (int rc = hamming_refusals(s, patterns, pattern_lens, n_patterns, k, who)) return rc;
  std::unique_ptr<sassy_hip_Result> R(new sassy_hip_Result());
  if (reads->n_records)
    if (int rc = hamming_reads_records(s, patterns, pattern_lens, n_patterns, reads_text(reads), reads->device, k,
                                       (flags & SASSY_HIP_WITHOUT_TRACE) != 0, R.get()))
      return rc;
  if (R->pool.empty()) R->pool.push_back('\0');
  *out = R.release();
  return 0;
}

int sassy_hip_hamming_best_pattern_reads(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                         const sassy_hip_Reads* reads, size_t k, uint32_t flags, uint8_t* out_cost, uint32_t* out_pattern,
                                         uint8_t* out_strand, uint64_t* out_start) {
  const char* who = "hamming_best_pattern_reads";
  if (int rc = reads_pointers(s, out_cost || (reads && reads->n_records == 0), patterns, pattern_lens, n_patterns, reads, who)) return rc;
  if (flags) return fail(SASSY_HIP_EINVAL, "hamming_best_pattern_reads takes no flags");
  if (k > 254) return fail(SASSY_HIP_EINVAL, "hamming_best_pattern_reads: k must be <= 254 (costs are bytes, 255 = no match)");
  if (int rc = hamming_refusals(s, patterns, pattern_lens, n_patterns, k, who)) return rc;
  // what the device cell cannot hold
  if (n_patterns >= (1u << 23))
    return fail(SASSY_HIP_EUNSUPPORTED, "hamming_best_pattern_reads takes fewer than 2^23 patterns (the cell keeps 2 pattern + strand in 24 bits)");
  if (reads->longest >= (1ull << 32))
    return fail(SASSY_HIP_EUNSUPPORTED, "hamming_best_pattern_reads takes reads shorter than 2^32 bytes (the cell keeps the start in 32 bits)");
  const size_t n_texts = reads->n_records;
  if (n_texts == 0) return 0;
  std::vector<unsigned long long> cells(n_texts, ~0ull);
  if (int rc = hamming_reads_cells(s, patterns, pattern_lens, n_patterns, reads_text(reads), reads->device, k, cells.data())) return rc;
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

int sassy_hip_hamming_counts_reads(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                   const sassy_hip_Reads* reads, size_t k, uint32_t flags, uint64_t* out_counts) {
  const char* who = "hamming_counts_reads";
  if (int rc = reads_pointers(s, out_counts != nullptr, patterns, pattern_lens, n_patterns, reads, who)) return rc;
  if (flags) return fail(SASSY_HIP_EINVAL, "hamming_counts_reads takes no flags");
  return hamming_reads_counts(s, patterns, pattern_lens, n_patterns, reads_text(reads), reads->device, k, who, out_counts);
}

}  // extern "C"
