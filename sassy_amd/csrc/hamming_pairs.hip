// hamming_pairs.hip -- all-vs-all Hamming distances between two sets of equal-length sequences, or inside one set
// (sassy_hip_hamming_pairs, sassy_hip_hamming_nearest; DESIGN.md 5.10 "Pairs").  There is no text: every sequence of A is
// compared with every sequence of B at the one alignment there is.  The arithmetic is pairs_step.h's.
//
// The host encodes both lists into bit planes (pairs_encode: Dna 2, Iupac 4, Ascii 8 planes of W = 1, 2 or 4 words) and an
// rc searcher's reverse complements of B as target records of their own, record r = S j + strand (S = 2, else 1): the
// kernels know nothing of strands.  A lane owns one entry of A with its planes in registers and walks the target records of
// its chunk in ascending r.  All lanes read the same record at the same time: the workgroup stages the records in tiles of
// 8 KiB in LDS and every lane reads them back as broadcasts (measured against scalar loads of the records: DESIGN.md).  Per
// record and lane: the mismatch word per 32 rows and a popcount that accumulates; per round of up to 8 records their
// minimum, one compare and one ballot-guarded branch -- everything else (the self-mode masks, the count, the minimum, the
// ties, the record store) lives behind that branch.
//
// Launches, grid = strips of 256 entries x chunks of targets (pairs_plan), no sort and no atomic anywhere:
//   pairs_survey_kernel   per (entry, chunk) one PairsCell -- candidates, smallest (cost, r), ties at it -- into the
//                         partials matrix [chunk][entry]
//   pairs_nearest_kernel  hamming_nearest: folds an entry's cells in chunk order (pairs_combine), writes the four columns
//   pairs_rows_kernel     hamming_pairs: per entry the place of every cell's first record in the entry's row, the row's sum
//   pairs_scan_*_kernel   the exclusive scan of the row sums, 64-bit: block sums, their scan by one workgroup, the rows
//   pairs_fill_kernel     walks again the tiles (wavefront x chunk) that hold a candidate and writes the records: a lane
//                         walks its targets in order and the cells are placed in (entry, chunk) order, so the records come
//                         out in the contract's order (a_idx, b_idx, strand)
//   pairs_cluster_kernel  hamming_clusters (clusters.hip): the survey's walk of the self-mode triangle, a union step per
//                         candidate (cluster_step.h) in place of the cell -- no matrix, no pass behind it here
// The passes between survey and fill know nothing of the distance: the host code around them (pairs_place_rows,
// pairs_take_records, pairs_fold_nearest; host_internal.h) also serves edit_pairs.hip, which has a walk of its own.
// Staging is two halves -- pairs_upload (encode, upload) and pairs_stage_resident (plan, arguments, grid) -- so that the walks
// also run over arrays a kernel made: umi_groups.hip gathers the distinct sequences of a list on the device and calls
// pairs_resident_link / pairs_resident_records on them, and scans its flags with pairs_scan_u64.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <stdexcept>
#include <system_error>
#include <thread>
#include <vector>

#include "cluster_step.h"
#include "host_internal.h"
#include "pairs_step.h"

namespace sassy_hip {
namespace {

static_assert(sizeof(PairsCell) == 16 && sizeof(sassy_hip_HammingPair) == 12, "cells are stored as uint4, records are 12 bytes");
static_assert(kPairsStrip == kWave * kWavesPerGroup && kPairsWave == kWave, "a strip is a workgroup, a tile a wavefront");

struct PairsArgs {
  const uint32_t* a;     // [n_a][P * W]
  const uint32_t* t;     // [S * n_b][P * W], record r = S j + strand
  uint64_t n_a, n_b;
  uint64_t chunk;        // targets per chunk
  uint32_t S, m, k, mode;
  uint4* cells;          // [n_chunks][n_a] PairsCell
  const unsigned long long* row_first;  // fill: per entry the index of its first record
  sassy_hip_HammingPair* out;
  uint32_t* parent;      // clusters: the forest of cluster_step.h, [n_a]
};

constexpr uint32_t kPairsTileWords = 2048;  // the staged tile: 8 KiB of records, 8 words per thread

// The walk of one lane over the targets of chunk c, shared by the survey and the fill: hit(r, j, strand, cost) for every
// candidate the call visits, in ascending r.  `a` holds the lane's planes; lanes beyond n_a walk along and never hit.  The
// whole workgroup calls it (it stages the tiles together); a wavefront with wave_active == false only helps staging.
template <int P, int W, bool IUPAC, typename Hit>
__device__ __forceinline__ void pairs_walk(const PairsArgs& A, uint64_t i, bool valid, bool wave_active, uint64_t c, const uint32_t (&a)[P * W], Hit&& hit) {
  constexpr int PW = P * W;
  constexpr int T = kPairsTileWords / PW;  // records per tile
  __shared__ uint32_t tile[kPairsTileWords];
  const uint64_t ib = (uint64_t)blockIdx.x * kPairsStrip;
  const uint64_t i0 = ib + (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(threadIdx.x / kWave)) * kPairsWave;
  const uint64_t j0 = pairs_chunk_begin(A.chunk, c), j1 = pairs_chunk_end(A.chunk, A.n_b, c);
  const uint32_t S = A.S, m = A.m, k = A.k, mode = A.mode;
  // the first record of the workgroup's walk and of this wavefront's: a self-mode tile starts at its own first entry
  // (records are counted in 64 bits: S n_b < 2^32, but a step of T beyond the last tile may not wrap)
  const uint64_t r_group = pairs_tile_first(mode, ib, j0, j1) * S, r_wave = pairs_tile_first(mode, i0, j0, j1) * S;
  const uint64_t r_end = j1 * S;
  auto candidate = [&](uint32_t r, uint32_t cost) {
    const uint32_t strand = S == 2 ? (r & 1u) : 0u;
    const uint64_t j = S == 2 ? (r >> 1) : r;
    if (valid && cost <= k && pairs_visits(mode, i, j, strand)) hit(r, j, strand, cost);
  };
  // U records per round, at most 32 words.  A round costs every lane the U distances, their minimum and ONE compare and
  // ballot-guarded branch; behind it the records are looked at one by one.
  constexpr int U = PW <= 4 ? 8 : 32 / PW;
  for (uint64_t rt = r_group; rt < r_end; rt += T) {
    const uint32_t cnt = r_end - rt < (uint64_t)T ? (uint32_t)(r_end - rt) : (uint32_t)T;
    __syncthreads();  // (the tile before this one has been read)
    uint32_t stage[kPairsTileWords / kPairsStrip];
#pragma unroll
    for (uint32_t e = 0; e < kPairsTileWords / kPairsStrip; ++e) {
      const uint32_t q = threadIdx.x + e * kPairsStrip;
      stage[e] = q < cnt * PW ? A.t[(size_t)rt * PW + q] : 0u;
    }
#pragma unroll
    for (uint32_t e = 0; e < kPairsTileWords / kPairsStrip; ++e) tile[threadIdx.x + e * kPairsStrip] = stage[e];
    __syncthreads();
    if (!wave_active) continue;
    uint32_t u = r_wave <= rt ? 0u : r_wave - rt < cnt ? (uint32_t)(r_wave - rt) : cnt;
    for (; u + U <= cnt; u += U) {
      uint32_t b[U * PW], cost[U];
#pragma unroll
      for (int q = 0; q < U * PW; ++q) b[q] = tile[u * PW + q];
#pragma unroll
      for (int v = 0; v < U; ++v) cost[v] = pairs_cost<P, W, IUPAC>(a, b + v * PW, m);
      uint32_t least = cost[0];
#pragma unroll
      for (int v = 1; v < U; ++v) least = cost[v] < least ? cost[v] : least;
      if (__ballot(least <= k) != 0ull) {  // rare
#pragma unroll
        for (int v = 0; v < U; ++v) candidate((uint32_t)(rt + u + v), cost[v]);
      }
    }
    for (; u < cnt; ++u) {  // (the last records of a chunk)
      uint32_t b[PW];
#pragma unroll
      for (int q = 0; q < PW; ++q) b[q] = tile[u * PW + q];
      const uint32_t cost = pairs_cost<P, W, IUPAC>(a, b, m);
      if (__ballot(cost <= k) != 0ull) candidate((uint32_t)(rt + u), cost);
    }
  }
}

template <int P, int W>
__device__ __forceinline__ void pairs_load_entry(const PairsArgs& A, uint64_t i, bool valid, uint32_t (&a)[P * W]) {
#pragma unroll
  for (int q = 0; q < P * W; ++q) a[q] = valid ? A.a[(size_t)i * (P * W) + q] : 0u;
}

template <int P, int W, bool IUPAC>
__global__ __launch_bounds__(kPairsStrip) void pairs_survey_kernel(PairsArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * kPairsStrip + threadIdx.x;
  const uint64_t c = blockIdx.y;
  const bool valid = i < A.n_a;
  uint32_t a[P * W];
  pairs_load_entry<P, W>(A, i, valid, a);
  PairsCell cell = pairs_empty_cell();
  pairs_walk<P, W, IUPAC>(A, i, valid, true, c, a, [&](uint32_t r, uint64_t, uint32_t, uint32_t cost) { cell = pairs_combine(cell, PairsCell{cost, r, 1u, 1u}); });
  if (valid) A.cells[c * A.n_a + i] = make_uint4(cell.cost, cell.r, cell.ties, cell.n_hits);
}

template <int P, int W, bool IUPAC>
__global__ __launch_bounds__(kPairsStrip) void pairs_fill_kernel(PairsArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * kPairsStrip + threadIdx.x;
  const uint64_t c = blockIdx.y;
  const bool valid = i < A.n_a;
  uint4 cell = make_uint4(0, 0, 0, 0);
  if (valid) cell = A.cells[c * A.n_a + i];
  const bool wave_active = __ballot(cell.w != 0u) != 0ull;  // (else: the tile holds no candidate)
  if (!__syncthreads_or(wave_active)) return;               // no tile of the strip does: nothing to stage
  uint32_t a[P * W];
  pairs_load_entry<P, W>(A, i, valid, a);
  uint64_t pos = valid ? A.row_first[i] + cell.z : 0;  // (cell.z: the place in the row, pairs_rows_kernel)
  pairs_walk<P, W, IUPAC>(A, i, valid, wave_active, c, a, [&](uint32_t, uint64_t j, uint32_t strand, uint32_t cost) {
    sassy_hip_HammingPair rec;
    rec.a_idx = (uint32_t)i; rec.b_idx = (uint32_t)j; rec.cost = (uint8_t)cost; rec.strand = (uint8_t)strand; rec.pad_[0] = rec.pad_[1] = 0;
    A.out[pos++] = rec;
  });
}

// hamming_clusters: the survey's walk over the self-mode triangle with a union step in place of the cell (cluster_step.h).
// j is the same for the whole wavefront, so the look at parent[j] that comes first is one broadcast load; a lane whose
// register already names j's parent goes on without a chase or a write.
template <int P, int W, bool IUPAC>
__global__ __launch_bounds__(kPairsStrip) void pairs_cluster_kernel(PairsArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * kPairsStrip + threadIdx.x;
  const uint64_t c = blockIdx.y;
  const bool valid = i < A.n_a;
  uint32_t a[P * W];
  pairs_load_entry<P, W>(A, i, valid, a);
  ClusterDeviceMem mem{A.parent};
  uint32_t root = (uint32_t)i;
  pairs_walk<P, W, IUPAC>(A, i, valid, true, c, a, [&](uint32_t, uint64_t j, uint32_t, uint32_t) {
    if (j != i) cluster_join(mem, (uint32_t)i, (uint32_t)j, root);  // ((i, i, 1) is no edge)
  });
}

// hamming_nearest: an entry's cells folded in chunk order -- the answer of one sequential walk
__global__ __launch_bounds__(256) void pairs_nearest_kernel(const uint4* cells, uint64_t n_a, uint32_t n_chunks, uint32_t S, uint8_t* out_cost,
                                                            uint32_t* out_index, uint8_t* out_strand, uint32_t* out_ties) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_a) return;
  PairsCell best = pairs_empty_cell();
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const uint4 v = cells[(uint64_t)c * n_a + i];
    best = pairs_combine(best, PairsCell{v.x, v.y, v.z, v.w});
  }
  const bool none = best.cost == kPairsNoCost;
  out_cost[i] = none ? (uint8_t)SASSY_HIP_NO_MATCH : (uint8_t)best.cost;
  out_index[i] = none ? 0xFFFFFFFFu : (S == 2 ? best.r >> 1 : best.r);
  out_strand[i] = none ? (uint8_t)0 : (uint8_t)(S == 2 ? best.r & 1u : 0u);
  out_ties[i] = none ? 0u : best.ties;
}

// hamming_pairs: per entry, every cell's `ties` becomes the place of its first record in the entry's row; the row's sum
__global__ __launch_bounds__(256) void pairs_rows_kernel(uint4* cells, uint64_t n_a, uint32_t n_chunks, unsigned long long* row_sum) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_a) return;
  unsigned long long run = 0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    uint4* cell = cells + (uint64_t)c * n_a + i;
    const uint32_t n = cell->w;
    cell->z = (uint32_t)run;  // (a row of 2^32 records or more: the call fails on the total)
    run += n;
  }
  row_sum[i] = run;
}

// ---- the exclusive scan of the row sums, 64-bit: kScanItems per thread, 256 threads ----
constexpr uint32_t kScanItems = 8, kScanBlock = 256 * kScanItems;
// inclusive Hillis-Steele over a workgroup's values; returns the exclusive value, *total the sum
template <int N>
__device__ unsigned long long pairs_group_scan(unsigned long long v, unsigned long long* lds, unsigned long long* total) {
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < (uint32_t)N; d <<= 1) {
    const unsigned long long add = t >= d ? lds[t - d] : 0ull;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  const unsigned long long incl = lds[t];
  *total = lds[N - 1];
  __syncthreads();
  return incl - v;
}
__global__ __launch_bounds__(256) void pairs_scan_sums_kernel(const unsigned long long* in, uint64_t n, unsigned long long* block_sum) {
  __shared__ unsigned long long lds[256];
  const uint64_t first = (uint64_t)blockIdx.x * kScanBlock + (uint64_t)threadIdx.x * kScanItems;
  unsigned long long v = 0;
  for (uint32_t q = 0; q < kScanItems; ++q)
    if (first + q < n) v += in[first + q];
  unsigned long long total;
  (void)pairs_group_scan<256>(v, lds, &total);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}
// one workgroup: block_sum[0 .. n_blocks) -> exclusive, in place; block_sum[n_blocks] = the total
__global__ __launch_bounds__(1024) void pairs_scan_top_kernel(unsigned long long* block_sum, uint64_t n_blocks) {
  __shared__ unsigned long long lds[1024];
  unsigned long long base = 0;
  for (uint64_t b0 = 0; b0 < n_blocks; b0 += 1024) {
    const uint64_t b = b0 + threadIdx.x;
    const unsigned long long v = b < n_blocks ? block_sum[b] : 0ull;
    unsigned long long total;
    const unsigned long long excl = pairs_group_scan<1024>(v, lds, &total);
    if (b < n_blocks) block_sum[b] = base + excl;
    base += total;
  }
  if (threadIdx.x == 0) block_sum[n_blocks] = base;
}
__global__ __launch_bounds__(256) void pairs_scan_rows_kernel(const unsigned long long* in, uint64_t n, const unsigned long long* block_first,
                                                              unsigned long long* out) {
  __shared__ unsigned long long lds[256];
  const uint64_t first = (uint64_t)blockIdx.x * kScanBlock + (uint64_t)threadIdx.x * kScanItems;
  unsigned long long item[kScanItems], v = 0;
  for (uint32_t q = 0; q < kScanItems; ++q) {
    item[q] = first + q < n ? in[first + q] : 0ull;
    v += item[q];
  }
  unsigned long long total;
  unsigned long long run = block_first[blockIdx.x] + pairs_group_scan<256>(v, lds, &total);
  for (uint32_t q = 0; q < kScanItems; ++q) {
    if (first + q < n) out[first + q] = run;
    run += item[q];
  }
}

// which kernel walks: the survey, the fill pass of hamming_pairs, the link pass of hamming_clusters
enum : int { kWalkSurvey = 0, kWalkFill = 1, kWalkCluster = 2 };
template <int P, bool IUPAC>
hipError_t launch_walk(int kind, uint32_t W, const PairsArgs& A, dim3 grid, hipStream_t st) {
  switch (W) {
    case 1:
      if (kind == kWalkCluster) hipLaunchKernelGGL((pairs_cluster_kernel<P, 1, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
      else if (kind == kWalkFill) hipLaunchKernelGGL((pairs_fill_kernel<P, 1, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
      else hipLaunchKernelGGL((pairs_survey_kernel<P, 1, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
      break;
    case 2:
      if (kind == kWalkCluster) hipLaunchKernelGGL((pairs_cluster_kernel<P, 2, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
      else if (kind == kWalkFill) hipLaunchKernelGGL((pairs_fill_kernel<P, 2, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
      else hipLaunchKernelGGL((pairs_survey_kernel<P, 2, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
      break;
    default:
      if (kind == kWalkCluster) hipLaunchKernelGGL((pairs_cluster_kernel<P, 4, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
      else if (kind == kWalkFill) hipLaunchKernelGGL((pairs_fill_kernel<P, 4, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
      else hipLaunchKernelGGL((pairs_survey_kernel<P, 4, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
      break;
  }
  return hipGetLastError();
}
hipError_t launch_walk_profile(Profile pr, int kind, uint32_t W, const PairsArgs& A, dim3 grid, hipStream_t st) {
  if (pr == PROFILE_DNA) return launch_walk<2, false>(kind, W, A, grid, st);
  if (pr == PROFILE_IUPAC) return launch_walk<4, true>(kind, W, A, grid, st);
  return launch_walk<8, false>(kind, W, A, grid, st);
}

// list[0 .. n) x m bytes -> planes, [n][S][P W] words: strand 1 of an entry (S = 2) is its reverse complement
void encode_list(Profile pr, const uint8_t* list, size_t n, uint32_t m, uint32_t W, uint32_t S, uint32_t* out) {
  const uint32_t PW = pairs_planes(pr) * W;
  auto slice = [&](size_t i0, size_t i1) {
    uint8_t rev[kPairsMaxRows];
    for (size_t i = i0; i < i1; ++i) {
      pairs_encode(pr, list + i * m, m, W, out + i * S * PW);
      if (S == 2) {
        pairs_reverse_complement(list + i * m, m, [&](uint8_t c) { return complement_char(pr, c); }, rev);
        pairs_encode(pr, rev, m, W, out + (i * S + 1) * PW);
      }
    }
  };
  pairs_for_slices(n, slice);
}

// A call behind its refusals: the plan, the walk's arguments, its grid.
struct PairsRun {
  PairsPlan plan;
  PairsArgs args{};
  uint32_t W = 1;
  dim3 grid;
};
// The second half of staging, for planes that lie on the device already (the lists a call uploaded, or arrays a kernel
// made: umi_groups.hip): the plan, the walk's arguments and grid, the stats' geometry.  d_a: [n_a][P W]; d_t: [S n_b][P W].
// want_cells: the partials matrix too (the clustering walk has none).
int pairs_stage_resident(sassy_SearcherType* s, const uint32_t* d_a, size_t n_a, const uint32_t* d_t, size_t n_b, bool self, uint32_t m, uint32_t k,
                         uint32_t self_mode, bool want_cells, PairsRun& R) {
  R.W = pairs_words(m);
  R.plan = pairs_plan(n_a, n_b, self ? self_mode : kPairsCross, s->sw.pairs_chunks, self_mode == kPairsSelfPairs ? kPairsFineChunk : 0);
  if (want_cells)
    if (int rc = s->d_pairs_cells.reserve((size_t)R.plan.n_chunks * n_a)) return rc;
  PairsArgs& A = R.args;
  A.a = d_a; A.t = d_t;
  A.n_a = n_a; A.n_b = n_b; A.chunk = R.plan.chunk;
  A.S = s->rc ? 2u : 1u; A.m = m; A.k = k; A.mode = R.plan.mode;
  A.cells = want_cells ? s->d_pairs_cells.p : nullptr;
  R.grid = dim3((uint32_t)R.plan.n_strips, R.plan.n_chunks);
  s->stats.scan_launches = 1;
  s->stats.chunks = R.plan.n_chunks;
  s->stats.grid = (uint32_t)R.plan.n_strips;
  s->stats.blocks_per_chunk = (uint32_t)std::min<uint64_t>(R.plan.chunk, 0xFFFFFFFFull);
  s->stats.text_bytes = (uint64_t)(n_a + n_b) * m;
  return 0;
}
// The first half: both lists encoded and uploaded (d_pairs_a: the entries; d_pairs_t: the target records, both strands of
// an rc searcher's).
int pairs_upload(sassy_SearcherType* s, const uint8_t* a, size_t n_a, const uint8_t* b, size_t n_b, uint32_t m) {
  hipStream_t st = s->stream;
  const bool self = b == nullptr;
  const uint32_t S = s->rc ? 2u : 1u, W = pairs_words(m), PW = pairs_planes(s->profile) * W;
  const size_t nb = self ? n_a : n_b;
  std::vector<uint32_t> ha(n_a * PW), ht(nb * S * PW);
  encode_list(s->profile, a, n_a, m, W, 1, ha.data());
  encode_list(s->profile, self ? a : b, nb, m, W, S, ht.data());
  if (int rc = s->d_pairs_a.reserve(ha.size())) return rc;
  if (int rc = s->d_pairs_t.reserve(ht.size())) return rc;
  HIP_TRY(hipMemcpyAsync(s->d_pairs_a.p, ha.data(), ha.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(s->d_pairs_t.p, ht.data(), ht.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));  // (the host vectors go away)
  return 0;
}
// A call behind its refusals, staged: upload, then the plan over what was uploaded.
int pairs_stage(sassy_SearcherType* s, const uint8_t* a, size_t n_a, const uint8_t* b, size_t n_b, uint32_t m, uint32_t k, uint32_t self_mode, bool want_cells,
                PairsRun& R) {
  if (int rc = pairs_upload(s, a, n_a, b, n_b, m)) return rc;
  return pairs_stage_resident(s, s->d_pairs_a.p, n_a, s->d_pairs_t.p, b ? n_b : n_a, b == nullptr, m, k, self_mode, want_cells, R);
}
// The survey: the partials matrix filled.
int pairs_survey(sassy_SearcherType* s, const uint8_t* a, size_t n_a, const uint8_t* b, size_t n_b, uint32_t m, uint32_t k, uint32_t self_mode, PairsRun& R) {
  hipStream_t st = s->stream;
  if (int rc = pairs_stage(s, a, n_a, b, n_b, m, k, self_mode, true, R)) return rc;
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[0], st));
  HIP_TRY(launch_walk_profile(s->profile, kWalkSurvey, R.W, R.args, R.grid, st));
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[1], st));
  s->stats.filtered = 8;
  return 0;
}
// Behind a survey: the rows placed, the total checked, the records written into d_pairs_out in the contract's order
// (*total == 0: none, and no fill pass).
int pairs_fill_records(sassy_SearcherType* s, PairsRun& R, const char* who, unsigned long long* total) {
  const unsigned long long* row_first = nullptr;
  if (int rc = pairs_place_rows(s, R.args.cells, R.args.n_a, R.plan.n_chunks, &row_first, total)) return rc;
  if (*total > 0xFFFFFFFFull) return fail(SASSY_HIP_ENOMEM, std::string(who) + ": more than 2^32 - 1 records (" + std::to_string(*total) + ")");
  if (*total == 0) return 0;
  if (int rc = s->d_pairs_out.reserve((size_t)*total * sizeof(sassy_hip_HammingPair))) return rc;
  R.args.row_first = row_first;
  R.args.out = reinterpret_cast<sassy_hip_HammingPair*>(s->d_pairs_out.p);
  HIP_TRY(launch_walk_profile(s->profile, kWalkFill, R.W, R.args, R.grid, s->stream));
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[3], s->stream));
  return 0;
}
}  // namespace

// What both entry points refuse, before any device work; self: b == NULL && n_b == 0.
int pairs_refusals(sassy_SearcherType* s, bool have_out, const uint8_t* a, size_t n_a, const uint8_t* b, size_t n_b, size_t m, size_t k, uint32_t flags,
                   const char* who) {
  const std::string w(who);
  if (!s || !a || !have_out) return fail(SASSY_HIP_EINVAL, "Pointers in " + w + "() must not be null");
  if (flags) return fail(SASSY_HIP_EINVAL, w + " takes no flags (the sequences are host bytes)");
  if (m == 0) return fail(SASSY_HIP_EINVAL, w + ": m must be at least 1");
  if (m > kPairsMaxRows) return fail(SASSY_HIP_EINVAL, w + ": m must be <= " + std::to_string(kPairsMaxRows) + " (got " + std::to_string(m) + ")");
  if (k > 254) return fail(SASSY_HIP_EINVAL, w + ": k must be <= 254 (the Hamming family's costs are bytes)");
  if (n_a == 0) return fail(SASSY_HIP_EINVAL, w + " needs at least one sequence in a");
  if (b && n_b == 0) return fail(SASSY_HIP_EINVAL, w + ": b is given but n_b is 0 (self mode is b == NULL and n_b == 0)");
  if (!b && n_b) return fail(SASSY_HIP_EINVAL, w + ": b is NULL but n_b is " + std::to_string(n_b));
  if (n_a > 0x7FFFFFFFull || n_b > 0x7FFFFFFFull)
    return fail(SASSY_HIP_EUNSUPPORTED, w + " takes at most 2^31 - 1 sequences per list (" + std::to_string(std::max(n_a, n_b)) + ")");
  if (!std::isnan(s->max_n_frac)) return fail(SASSY_HIP_EUNSUPPORTED, w + " does not take max_n_frac: there is no text span for it to apply to");
  // the family's own checks, on each list as it stands: the sequences are its patterns, so "pattern N" in its messages is
  // sequence N of the list named behind the message
  auto family = [&](const uint8_t* list, size_t n, const char* name) {
    std::vector<const uint8_t*> seqs(n);
    for (size_t i = 0; i < n; ++i) seqs[i] = list + i * m;
    const std::vector<size_t> lens(n, m);
    const int rc = hamming_refusals(s, seqs.data(), lens.data(), n, k, who);
    if (rc) g_err += std::string(" (") + who + ": list " + name + ")";
    return rc;
  };
  if (int rc = family(a, n_a, "a")) return rc;
  return b ? family(b, n_b, "b") : 0;
}

// hamming_clusters (clusters.hip): the list staged as a self-mode pairs call stages it, one launch of the link kernel
int pairs_link_components(sassy_SearcherType* s, const uint8_t* a, size_t n, uint32_t m, uint32_t k, uint32_t* d_parent) {
  hipStream_t st = s->stream;
  PairsRun R;
  if (int rc = pairs_stage(s, a, n, nullptr, 0, m, k, kPairsSelfPairs, false, R)) return rc;
  R.args.parent = d_parent;
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[0], st));
  HIP_TRY(launch_walk_profile(s->profile, kWalkCluster, R.W, R.args, R.grid, st));
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[1], st));
  return 0;
}

// ---- what umi_groups.hip uses (host_internal.h): the list's upload alone, then the walks over arrays that a kernel made ----
// The list as a self-mode call stages it: *d_a [n][P W], *d_t [S n][P W] (d_pairs_a, d_pairs_t).
int pairs_upload_self(sassy_SearcherType* s, const uint8_t* a, size_t n, uint32_t m, const uint32_t** d_a, const uint32_t** d_t) {
  if (int rc = pairs_upload(s, a, n, nullptr, 0, m)) return rc;
  *d_a = s->d_pairs_a.p;
  *d_t = s->d_pairs_t.p;
  return 0;
}
// The link pass of the clustering call over n device-resident entries and their target records: no event, no copy.
int pairs_resident_link(sassy_SearcherType* s, const uint32_t* d_a, const uint32_t* d_t, size_t n, uint32_t m, uint32_t k, uint32_t* d_parent) {
  PairsRun R;
  if (int rc = pairs_stage_resident(s, d_a, n, d_t, n, true, m, k, kPairsSelfPairs, false, R)) return rc;
  R.args.parent = d_parent;
  HIP_TRY(launch_walk_profile(s->profile, kWalkCluster, R.W, R.args, R.grid, s->stream));
  return 0;
}
// The self-mode records of n device-resident entries: survey, rows, scan, fill.  They stay in d_pairs_out, *total of them
// (stats.candidates too); more than 2^32 - 1: SASSY_HIP_ENOMEM with the count, as the pair call fails.
int pairs_resident_records(sassy_SearcherType* s, const uint32_t* d_a, const uint32_t* d_t, size_t n, uint32_t m, uint32_t k, const char* who,
                           unsigned long long* total) {
  PairsRun R;
  if (int rc = pairs_stage_resident(s, d_a, n, d_t, n, true, m, k, kPairsSelfPairs, true, R)) return rc;
  HIP_TRY(launch_walk_profile(s->profile, kWalkSurvey, R.W, R.args, R.grid, s->stream));
  if (int rc = pairs_fill_records(s, R, who, total)) return rc;
  s->stats.scan_launches = *total ? 2 : 1;
  return 0;
}

// ---- what edit_pairs.hip shares (host_internal.h): the passes behind a survey that do not depend on the distance ----
// slice(i0, i1) over [0, n) in up to 8 host threads (a list of a million sequences is encoded in a fraction of the time)
void pairs_for_slices(size_t n, const std::function<void(size_t, size_t)>& slice) {
  const size_t workers = n < (1u << 16) ? 1 : std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency()));
  if (workers == 1) return slice(0, n);
  std::vector<std::thread> pool;
  pool.reserve(workers);
  size_t w = 0;
  try {
    for (; w + 1 < workers; ++w) pool.emplace_back(slice, n * w / workers, n * (w + 1) / workers);
  } catch (const std::system_error&) {  // (no more threads to be had: this one does the rest)
  }
  slice(n * w / workers, n);
  for (std::thread& t : pool) t.join();
}
// timing level 2: filter_ms the survey, trace_ms the last pass (fill or reduce), scan_ms all of it -- the scan between them
void pairs_times(sassy_SearcherType* s, bool has_last) {
  if (s->timing < 2) return;
  float survey = 0, mid = 0, last = 0;
  (void)hipEventElapsedTime(&survey, s->ev_line[0], s->ev_line[1]);
  (void)hipEventElapsedTime(&mid, s->ev_line[1], s->ev_line[2]);
  if (has_last) (void)hipEventElapsedTime(&last, s->ev_line[2], s->ev_line[3]);
  s->stats.filter_ms = survey;
  s->stats.trace_ms = last;
  s->stats.scan_ms = (double)survey + mid + last;
}
// The 64-bit exclusive scan of in[0 .. n) into out, on the searcher's stream: block sums, their scan by one workgroup, the
// items.  block_sum: pairs_scan_blocks(n) + 1 entries of the caller's; the total is left in its last one.
uint64_t pairs_scan_blocks(uint64_t n) { return (n + kScanBlock - 1) / kScanBlock; }
int pairs_scan_u64(sassy_SearcherType* s, const unsigned long long* in, uint64_t n, unsigned long long* block_sum, unsigned long long* out) {
  hipStream_t st = s->stream;
  const uint64_t n_blocks = pairs_scan_blocks(n);
  hipLaunchKernelGGL(pairs_scan_sums_kernel, dim3((uint32_t)n_blocks), dim3(256), 0, st, in, n, block_sum);
  hipLaunchKernelGGL(pairs_scan_top_kernel, dim3(1), dim3(1024), 0, st, block_sum, n_blocks);
  hipLaunchKernelGGL(pairs_scan_rows_kernel, dim3((uint32_t)n_blocks), dim3(256), 0, st, in, n, block_sum, out);
  HIP_TRY(hipGetLastError());
  return 0;
}
// the rows' sums, their exclusive scan, the total: every cell's place in its row, *row_first the device's table of rows
int pairs_place_rows(sassy_SearcherType* s, uint4* cells, uint64_t n_a, uint32_t n_chunks, const unsigned long long** row_first_out,
                     unsigned long long* total_out) {
  hipStream_t st = s->stream;
  const uint64_t n_blocks = pairs_scan_blocks(n_a);
  if (int rc = s->d_pairs_rows.reserve(2 * n_a + n_blocks + 1)) return rc;
  unsigned long long *row_sum = s->d_pairs_rows.p, *row_first = row_sum + n_a, *block_sum = row_first + n_a;
  const uint32_t row_grid = (uint32_t)((n_a + 255) / 256);
  hipLaunchKernelGGL(pairs_rows_kernel, dim3(row_grid), dim3(256), 0, st, cells, n_a, n_chunks, row_sum);
  if (int rc = pairs_scan_u64(s, row_sum, n_a, block_sum, row_first)) return rc;
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[2], st));
  unsigned long long total = 0;
  HIP_TRY(hipMemcpyAsync(&total, block_sum + n_blocks, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s->stats.candidates = total;
  *row_first_out = row_first;
  *total_out = total;
  return 0;
}
// the `total` records a fill pass left in d_pairs_out, as the caller's malloc'd array
int pairs_take_records(sassy_SearcherType* s, unsigned long long total, sassy_hip_HammingPair** out, size_t* n_out) {
  hipStream_t st = s->stream;
  sassy_hip_HammingPair* p = static_cast<sassy_hip_HammingPair*>(malloc((size_t)total * sizeof(sassy_hip_HammingPair)));
  if (!p) return fail(SASSY_HIP_ENOMEM, "out of host memory (pair records)");
  std::unique_ptr<sassy_hip_HammingPair, decltype(&free)> hold(p, &free);
  HIP_TRY(hipMemcpyAsync(p, s->d_pairs_out.p, (size_t)total * sizeof(sassy_hip_HammingPair), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  pairs_times(s, true);
  *out = hold.release();
  *n_out = (size_t)total;
  return 0;
}
// nearest: every entry's cells folded on the device, the four columns (index | ties | cost | strand) to the caller's arrays
int pairs_fold_nearest(sassy_SearcherType* s, const uint4* cells, uint64_t n_a, uint32_t n_chunks, uint32_t S, uint8_t* out_cost, uint32_t* out_index,
                       uint8_t* out_strand, uint32_t* out_ties) {
  hipStream_t st = s->stream;
  if (int rc = s->d_pairs_out.reserve(n_a * 10)) return rc;
  uint32_t *d_index = reinterpret_cast<uint32_t*>(s->d_pairs_out.p), *d_ties = d_index + n_a;
  uint8_t *d_cost = reinterpret_cast<uint8_t*>(d_ties + n_a), *d_strand = d_cost + n_a;
  hipLaunchKernelGGL(pairs_nearest_kernel, dim3((uint32_t)((n_a + 255) / 256)), dim3(256), 0, st, cells, n_a, n_chunks, S, d_cost, d_index, d_strand,
                     d_ties);
  HIP_TRY(hipGetLastError());
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[2], st));
  HIP_TRY(hipMemcpyAsync(out_cost, d_cost, n_a, hipMemcpyDeviceToHost, st));
  if (out_index) HIP_TRY(hipMemcpyAsync(out_index, d_index, n_a * 4, hipMemcpyDeviceToHost, st));
  if (out_strand) HIP_TRY(hipMemcpyAsync(out_strand, d_strand, n_a, hipMemcpyDeviceToHost, st));
  if (out_ties) HIP_TRY(hipMemcpyAsync(out_ties, d_ties, n_a * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  pairs_times(s, false);
  return 0;
}

}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_hamming_pairs(sassy_SearcherType* s, const uint8_t* a, size_t n_a, const uint8_t* b, size_t n_b, size_t m, size_t k, uint32_t flags,
                            sassy_hip_HammingPair** out, size_t* n_out) {
  const char* who = "hamming_pairs";
  return pairs_guarded(who, [&]() -> int {
  if (int rc = pairs_refusals(s, out && n_out, a, n_a, b, n_b, m, k, flags, who)) return rc;
  *out = nullptr;
  *n_out = 0;
  const size_t lens[1] = {m};
  return hamming_call(s, lens, 1, k, [&](uint32_t kk) {  // (k >= m: every pair is a record)
    PairsRun R;
    if (int rc = pairs_survey(s, a, n_a, b, n_b, (uint32_t)m, kk, kPairsSelfPairs, R)) return rc;
    unsigned long long total = 0;
    if (int rc = pairs_fill_records(s, R, who, &total)) return rc;
    if (total == 0) {
      pairs_times(s, false);
      return 0;
    }
    s->stats.scan_launches = 2;
    return pairs_take_records(s, total, out, n_out);
  });
  });
}

void sassy_hip_hamming_pairs_free(sassy_hip_HammingPair* p) { free(p); }

int sassy_hip_hamming_nearest(sassy_SearcherType* s, const uint8_t* a, size_t n_a, const uint8_t* b, size_t n_b, size_t m, size_t k, uint32_t flags,
                              uint8_t* out_cost, uint32_t* out_index, uint8_t* out_strand, uint32_t* out_ties) {
  const char* who = "hamming_nearest";
  return pairs_guarded(who, [&]() -> int {
  if (int rc = pairs_refusals(s, out_cost != nullptr, a, n_a, b, n_b, m, k, flags, who)) return rc;
  const size_t lens[1] = {m};
  return hamming_call(s, lens, 1, k, [&](uint32_t kk) {
    PairsRun R;
    if (int rc = pairs_survey(s, a, n_a, b, n_b, (uint32_t)m, kk, kPairsSelfNearest, R)) return rc;
    return pairs_fold_nearest(s, R.args.cells, n_a, R.plan.n_chunks, R.args.S, out_cost, out_index, out_strand, out_ties);
  });
  });
}

}  // extern "C"
