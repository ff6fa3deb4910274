// line_index.hip -- line resolution on the device: positions in a resident text -> line number, line start, line end.
//
// '\n' (0x0A) is the only separator.  For a position p of a text t of n bytes:
//   line_no(p)    = 1 + the number of '\n' in t[0:p]
//   line_start(p) = 1 + the index of the last '\n' in t[0:p], 0 if there is none
//   line_end(p)   = the index of the first '\n' in t[p:n], n if there is none
// A span [first, last] gets {line_no(first), line_no(last), line_start(first), line_end(last)} (sassy_hip_LineSpan).
//
// The index has two levels, so that only the upper one needs 64-bit sums and its scan stays small:
//   tile       = kLineTile = 4 KiB of text: what one wave scans in one step (four 16-byte loads per lane: 1 KiB of
//                consecutive bytes per load instruction in the counting pass, 64 consecutive bytes per lane in the resolve
//                pass, which needs the newlines in order); the resolve pass scans one or two tiles per span end, so a
//                span costs the same whatever the length of its line.  tile_off[i] (u32) = newlines in front of tile i INSIDE its super-tile.
//   super-tile = kLineSuper = 16 tiles = 64 KiB: what one workgroup of line_count_kernel counts.  super_prefix[s] (u64) =
//                newlines in front of super-tile s; super_prefix[n_super] = all of them.  3 GB of text: 46 000 entries.
// Launches: line_count_kernel (reads the text once, 16-byte loads, memory-bound) and line_scan_kernel (one workgroup: the
// exclusive scan of the super-tile counts) build the index; line_resolve_kernel gives every span a wave.  "Newline number
// c" (1-based) is found by a binary search over super_prefix, one over the <= 16 tile offsets of that super-tile, and a
// scan of that one tile -- unless it lies in the tile of the position itself, which the wave has in registers anyway.
#include "host_internal.h"

namespace sassy_hip {

namespace {

constexpr uint32_t kLineTile = SASSY_HIP_LINE_TILE;
constexpr uint32_t kLineTilesPerSuper = 16;
constexpr uint32_t kLineSuper = kLineTile * kLineTilesPerSuper;
static_assert(kLineTile == 64 * 64, "a tile is 64 lanes x 64 bytes");

// bit b of the result: byte b of v is '\n'
__device__ __forceinline__ uint32_t newline_bits4(uint32_t v) {
  const uint32_t z = v ^ 0x0A0A0A0Au;
  const uint32_t t = ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;  // bit 7 of every zero byte of z, exactly
  // bits 0, 8, 16, 24 -> bits 21 .. 24: the products 2^(8i + 7j) are all distinct, i + j = 3 lands on 21 + i
  return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}
__device__ __forceinline__ uint32_t newline_bits16(const uint4 v) {
  return newline_bits4(v.x) | newline_bits4(v.y) << 4 | newline_bits4(v.z) << 8 | newline_bits4(v.w) << 12;
}

// The lane's 64 bytes of a tile, [tile * kLineTile + 64 lane, + 64): bit b = byte b is '\n'.  Bytes at n and behind read
// as "no newline".  The text is 16-byte aligned and readable up to the next multiple of 64 behind n (the contract of
// SASSY_HIP_TEXT_ON_DEVICE; an uploaded text has 64 spare bytes), so a 16-byte load that starts in front of n is legal.
__device__ __forceinline__ uint64_t lane_newlines(const uint8_t* text, uint64_t n, uint64_t tile, uint32_t lane) {
  const uint64_t base = tile * kLineTile + 64ull * lane;
  uint4 v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = make_uint4(0u, 0u, 0u, 0u);
    if (base + 16u * j < n) v[j] = *reinterpret_cast<const uint4*>(text + base + 16u * j);
  }
  uint64_t mask = (uint64_t)newline_bits16(v[0]) | (uint64_t)newline_bits16(v[1]) << 16 |
                  (uint64_t)newline_bits16(v[2]) << 32 | (uint64_t)newline_bits16(v[3]) << 48;
  if (base >= n) mask = 0;
  else if (n - base < 64) mask &= (1ull << (n - base)) - 1ull;
  return mask;
}

// Newlines of a tile for the counting pass, where their order does not matter: lane l takes bytes [1024 j + 16 l, + 16) of
// the tile, j = 0 .. 3 -- every load instruction of the wave reads 1 KiB of consecutive bytes.
__device__ __forceinline__ uint32_t lane_newline_count(const uint8_t* text, uint64_t n, uint64_t tile, uint32_t lane) {
  const uint64_t base = tile * kLineTile + 16ull * lane;
  uint4 v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = make_uint4(0u, 0u, 0u, 0u);
    if (base + 1024u * j < n) v[j] = *reinterpret_cast<const uint4*>(text + base + 1024u * j);
  }
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t bits = newline_bits16(v[j]);
    const uint64_t at = base + 1024u * j;
    if (at >= n) bits = 0;
    else if (n - at < 16) bits &= (1u << (uint32_t)(n - at)) - 1u;
    c += (uint32_t)__popc(bits);
  }
  return c;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
  return v;
}

// Pass one: a workgroup per super-tile, a wave per four of its tiles.
__global__ __launch_bounds__(256) void line_count_kernel(const uint8_t* text, uint64_t n, uint64_t n_tiles, uint32_t* tile_off,
                                                         uint32_t* super_count) {
  __shared__ uint32_t counts[kLineTilesPerSuper];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t tile0 = (uint64_t)blockIdx.x * kLineTilesPerSuper;
#pragma unroll
  for (uint32_t i = 0; i < kLineTilesPerSuper / 4; ++i) {
    const uint32_t t = wave * (kLineTilesPerSuper / 4) + i;
    const uint32_t c = wave_sum(lane_newline_count(text, n, tile0 + t, lane));
    if (lane == 0) counts[t] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (uint32_t t = 0; t < kLineTilesPerSuper; ++t) {
      if (tile0 + t < n_tiles) tile_off[tile0 + t] = run;
      run += counts[t];
    }
    super_count[blockIdx.x] = run;
  }
}

// Exclusive scan of the super-tile counts, 64-bit sums: one workgroup, a contiguous run of entries per thread.
// super_prefix has n_super + 1 entries.
__global__ __launch_bounds__(1024) void line_scan_kernel(const uint32_t* super_count, uint64_t n_super, unsigned long long* super_prefix) {
  __shared__ unsigned long long sums[1024];
  const uint64_t per = (n_super + 1023) / 1024;
  const uint64_t lo = min((uint64_t)threadIdx.x * per, n_super), hi = min(lo + per, n_super);
  unsigned long long mine = 0;
  for (uint64_t i = lo; i < hi; ++i) mine += super_count[i];
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
    super_prefix[i] = run;
    run += super_count[i];
  }
  if (threadIdx.x == 1023) super_prefix[n_super] = sums[1023];
}

struct LineIndexView {
  const uint8_t* text;
  uint64_t n, n_tiles, n_super;
  const uint32_t* tile_off;
  const unsigned long long* super_prefix;
};

// What a wave knows about a position once it has scanned the position's tile.
struct PosInfo {
  uint64_t before;    // newlines in t[0:p]
  uint64_t tile;      // p's tile (n_tiles for p == n on a tile border)
  uint32_t last_nl;   // offset in the tile of the last newline in front of p, 0xFFFFFFFF if the tile has none there
  uint32_t next_nl;   // offset in the tile of the first newline at p or behind it, 0xFFFFFFFF if the tile has none
};

__device__ __forceinline__ PosInfo look_at(const LineIndexView& X, uint64_t p, uint32_t lane) {
  PosInfo r;
  r.tile = p / kLineTile;
  r.last_nl = r.next_nl = 0xFFFFFFFFu;
  if (r.tile >= X.n_tiles) {  // p == n, and n is a multiple of the tile (or 0)
    r.before = X.super_prefix[X.n_super];
    return r;
  }
  const uint64_t mask = lane_newlines(X.text, X.n, r.tile, lane);
  const uint32_t off = (uint32_t)(p - r.tile * kLineTile);  // 0 .. 4095
  const uint32_t mine = 64u * lane;
  // the lane's bits in front of p / at p and behind
  const uint64_t below = off <= mine ? 0ull : off - mine >= 64u ? ~0ull : (1ull << (off - mine)) - 1ull;
  const uint64_t lo = mask & below, hi = mask & ~below;
  const uint32_t in_tile = wave_sum((uint32_t)__popcll(lo));
  const uint32_t last = wave_max(lo ? mine + 63u - (uint32_t)__clzll((long long)lo) + 1u : 0u);  // offset + 1, 0 = none
  r.next_nl = wave_min(hi ? mine + (uint32_t)__ffsll((unsigned long long)hi) - 1u : 0xFFFFFFFFu);
  r.last_nl = last ? last - 1u : 0xFFFFFFFFu;
  r.before = X.super_prefix[r.tile / kLineTilesPerSuper] + X.tile_off[r.tile] + in_tile;
  return r;
}

// Position of newline number c (1 <= c <= all newlines) of the text.
__device__ __forceinline__ uint64_t find_newline(const LineIndexView& X, uint64_t c, uint32_t lane) {
  // the last super-tile with fewer than c newlines in front of it
  uint64_t lo = 0, hi = X.n_super - 1;
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (X.super_prefix[mid] < c) lo = mid;
    else hi = mid - 1;
  }
  const uint32_t r = (uint32_t)(c - X.super_prefix[lo]);  // 1 .. 65536: its rank inside the super-tile
  const uint64_t t0 = lo * kLineTilesPerSuper;
  uint32_t tl = 0, th = (uint32_t)min((uint64_t)kLineTilesPerSuper, X.n_tiles - t0) - 1u;
  while (tl < th) {
    const uint32_t mid = (tl + th + 1u) >> 1;
    if (X.tile_off[t0 + mid] < r) tl = mid;
    else th = mid - 1u;
  }
  const uint64_t tile = t0 + tl;
  const uint32_t want = r - X.tile_off[tile];  // 1 .. 4096: its rank inside the tile
  uint64_t mask = lane_newlines(X.text, X.n, tile, lane);
  const uint32_t cnt = (uint32_t)__popcll(mask);
  uint32_t incl = cnt;  // inclusive prefix sum over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if ((int)lane >= o) incl += up;
  }
  const uint32_t excl = incl - cnt;
  uint32_t found = 0xFFFFFFFFu;
  if (excl < want && want <= incl) {  // exactly one lane
    for (uint32_t i = excl + 1; i < want; ++i) mask &= mask - 1ull;
    found = 64u * lane + (uint32_t)__ffsll((unsigned long long)mask) - 1u;
  }
  return tile * kLineTile + wave_min(found);
}

// Pass two: a wave per span.
__global__ __launch_bounds__(256) void line_resolve_kernel(LineIndexView X, const uint64_t* first, const uint64_t* last, uint64_t n_spans,
                                                           sassy_hip_LineSpan* out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
  const uint64_t total = X.super_prefix[X.n_super];
  for (uint64_t i = wave; i < n_spans; i += n_waves) {
    const uint64_t a = first[i], b = last[i];
    const PosInfo A = look_at(X, a, lane);
    const PosInfo B = a == b ? A : look_at(X, b, lane);
    uint64_t start = 0, end = X.n;
    if (A.before != 0)
      start = (A.last_nl != 0xFFFFFFFFu ? A.tile * kLineTile + A.last_nl : find_newline(X, A.before, lane)) + 1;
    if (B.before < total)
      end = B.next_nl != 0xFFFFFFFFu ? B.tile * kLineTile + B.next_nl : find_newline(X, B.before + 1, lane);
    if (lane == 0) {
      sassy_hip_LineSpan r;
      r.line_no = A.before + 1;
      r.last_line_no = B.before + 1;
      r.line_start = start;
      r.line_end = end;
      out[i] = r;
    }
  }
}

}  // namespace

// The spans of `n` (first, last) pairs (host arrays, already validated) over the device text d_text[0 .. text_len).
int line_spans_on_device(sassy_SearcherType* S, const uint8_t* d_text, uint64_t text_len, const uint64_t* first, const uint64_t* last,
                         size_t n, sassy_hip_LineSpan* out) {
  if (n == 0) return 0;
  if (text_len == 0) {  // one empty line
    for (size_t i = 0; i < n; ++i) out[i] = sassy_hip_LineSpan{1, 1, 0, 0};
    return 0;
  }
  const uint64_t n_tiles = (text_len + kLineTile - 1) / kLineTile, n_super = (text_len + kLineSuper - 1) / kLineSuper;
  if (n_super > 0x7FFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "text too long for the line index");
  if (int rc = S->d_line_tiles.reserve(n_tiles + n_super)) return rc;
  if (int rc = S->d_line_prefix.reserve(n_super + 1)) return rc;
  if (int rc = S->d_line_pos.reserve(2 * n)) return rc;
  if (int rc = S->d_line_out.reserve(n)) return rc;
  uint32_t* tile_off = S->d_line_tiles.p;
  uint32_t* super_count = S->d_line_tiles.p + n_tiles;
  hipStream_t st = S->stream;
  const bool timed = S->timing >= 2;
  LineIndexView X{d_text, text_len, n_tiles, n_super, tile_off, S->d_line_prefix.p};
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 3) / 4, 16384);
  // every step is queued through `le`; whatever fails, the stream is drained before the caller's arrays are let go
  hipError_t le = hipSuccess;
  auto step = [&](hipError_t e) { if (le == hipSuccess) le = e; return le == hipSuccess; };
  if (timed) step(hipEventRecord(S->ev_line[0], st));
  if (le == hipSuccess) {
    hipLaunchKernelGGL(line_count_kernel, dim3((uint32_t)n_super), dim3(256), 0, st, d_text, text_len, n_tiles, tile_off, super_count);
    step(hipGetLastError());
  }
  if (le == hipSuccess) {
    hipLaunchKernelGGL(line_scan_kernel, dim3(1), dim3(1024), 0, st, super_count, n_super, S->d_line_prefix.p);
    step(hipGetLastError());
  }
  if (timed && le == hipSuccess) step(hipEventRecord(S->ev_line[1], st));
  if (le == hipSuccess) step(hipMemcpyAsync(S->d_line_pos.p, first, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (le == hipSuccess) step(hipMemcpyAsync(S->d_line_pos.p + n, last, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (timed && le == hipSuccess) step(hipEventRecord(S->ev_line[2], st));
  if (le == hipSuccess) {
    hipLaunchKernelGGL(line_resolve_kernel, dim3(grid), dim3(256), 0, st, X, (const uint64_t*)S->d_line_pos.p,
                       (const uint64_t*)(S->d_line_pos.p + n), (uint64_t)n, S->d_line_out.p);
    step(hipGetLastError());
  }
  if (timed && le == hipSuccess) step(hipEventRecord(S->ev_line[3], st));
  if (le == hipSuccess) step(hipMemcpyAsync(out, S->d_line_out.p, n * sizeof(sassy_hip_LineSpan), hipMemcpyDeviceToHost, st));
  const hipError_t se = hipStreamSynchronize(st);
  step(se);
  if (timed && le == hipSuccess) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, S->ev_line[0], S->ev_line[1]) == hipSuccess) S->line_index_ms = ms;
    if (hipEventElapsedTime(&ms, S->ev_line[2], S->ev_line[3]) == hipSuccess) S->line_resolve_ms = ms;
  }
  if (le != hipSuccess) return hip_fail(le, "line spans");
  return 0;
}

}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

uint32_t sassy_hip_line_tile(void) { return kLineTile; }

int sassy_hip_line_spans(sassy_SearcherType* s, const void* text, size_t text_len, uint32_t flags, const uint64_t* first,
                         const uint64_t* last, size_t n, sassy_hip_LineSpan* out) {
  if (!s || (!text && text_len) || (n && (!first || !last || !out))) return fail(SASSY_HIP_EINVAL, "null argument");
  if (flags & ~SASSY_HIP_TEXT_ON_DEVICE) return fail(SASSY_HIP_EINVAL, "line_spans takes SASSY_HIP_TEXT_ON_DEVICE only");
  SASSY_NO_TICKETS(s);
  for (size_t i = 0; i < n; ++i)
    if (first[i] > last[i] || last[i] > text_len) return fail(SASSY_HIP_EINVAL, "span " + std::to_string(i) + " is not first <= last <= text_len");
  if (n == 0) return 0;
  DeviceGuard on_device(s);
  if (int rc = s->ensure_device()) return rc;
  const uint8_t* d_text = static_cast<const uint8_t*>(text);
  if (flags & SASSY_HIP_TEXT_ON_DEVICE) {
    if (((uintptr_t)text & 15) != 0) return fail(SASSY_HIP_EINVAL, "device text pointer must be 16-byte aligned");
  } else if (text_len) {
    if (int rc = s->d_text.reserve(text_len + 64)) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_text.p, text, text_len, hipMemcpyHostToDevice, s->stream));
    d_text = s->d_text.p;
  }
  return line_spans_on_device(s, d_text, text_len, first, last, n, out);
}

/* HIP-event times of the last line-span call's two passes (timing level 2; tools/bench_lines.py) */
int sassy_hip_line_span_times(const sassy_SearcherType* s, double* index_ms, double* resolve_ms) {
  if (!s || !index_ms || !resolve_ms) return fail(SASSY_HIP_EINVAL, "null argument");
  *index_ms = s->line_index_ms;
  *resolve_ms = s->line_resolve_ms;
  return 0;
}

}  // extern "C"
