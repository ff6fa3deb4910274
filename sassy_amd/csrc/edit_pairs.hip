// edit_pairs.hip -- all-vs-all edit (Levenshtein) distances between two sets of sequences, or inside one set
// (sassy_hip_edit_pairs, sassy_hip_edit_nearest; DESIGN.md 5.10 "Edit pairs").  The contract is the Hamming pair calls' with
// E in place of H; the two lists may have lengths of their own, m_a and m_b <= 64.  The arithmetic is edit_pairs_step.h's.
//
// The shape is hamming_pairs.hip's.  The host encodes the entries of A into pairs_encode's bit planes and the targets into
// records of packed row codes, an rc searcher's reverse complements as records of their own, r = S j + strand.  A lane owns
// one entry with its planes in registers and walks the records of its chunk in ascending r; the workgroup stages them in
// tiles of 8 KiB in LDS and every lane reads them back as broadcasts.  A record's codes are the same for the whole
// wavefront: a word of them is made scalar once (readfirstlane) and taken apart column by column on the scalar unit, so the
// vector unit sees nothing but the Eq word and the column step.  A lane steps U records at a time, column by column side by
// side -- U independent chains of a dozen dependent operations each -- and their costs share one compare and one
// ballot-guarded branch; the self-mode masks, the cell and the record store live behind it.
//
// Launches, grid = strips of 256 entries x chunks of targets (pairs_plan; pairs_chunks forces the chunk count):
//   edit_survey_kernel   per (entry, chunk) one PairsCell into the partials matrix [chunk][entry]
//   edit_fill_kernel     edit_pairs: walks again the tiles (wavefront x chunk) that hold a candidate and writes the records
//   edit_cluster_kernel  edit_clusters (clusters.hip): the survey's walk of the self-mode triangle, a union step per
//                        candidate (cluster_step.h) in place of the cell
// and between them the passes that know nothing of the distance, which exist once, in hamming_pairs.hip (pairs_fold_nearest;
// pairs_place_rows, pairs_take_records).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "cluster_step.h"
#include "edit_pairs_step.h"
#include "host_internal.h"

namespace sassy_hip {
namespace {

static_assert(sizeof(sassy_hip_EditPair) == 12, "records are 12 bytes");
static_assert(kPairsStrip == kWave * kWavesPerGroup && kPairsWave == kWave, "a strip is a workgroup, a tile a wavefront");

struct EditArgs {
  const uint32_t* a;     // [n_a][P * W] planes
  const uint32_t* t;     // [S * n_b][rw] row codes, record r = S j + strand
  uint64_t n_a, n_b;
  uint64_t chunk;        // targets per chunk
  uint32_t S, m_a, m_b, rw, k, mode;
  uint4* cells;          // [n_chunks][n_a] PairsCell
  const unsigned long long* row_first;  // fill: per entry the index of its first record
  sassy_hip_EditPair* out;
  uint32_t* parent;      // clusters: the forest of cluster_step.h, [n_a]
};

constexpr uint32_t kEditTileWords = 2048;  // the staged tile: 8 KiB of records, 8 words per thread; a record is at most 16 words

// E of the lane's entry against U records that lie back to back in LDS, stepped side by side.
template <int P, int W, bool IUPAC, int U>
__device__ __forceinline__ void edit_round(const EditWord<W> (&a)[P], const uint32_t* rec, uint32_t rw, uint32_t m_b, EditWord<W> rows, uint32_t (&cost)[U]) {
  constexpr uint32_t kCols = 32 / P;
  EditWord<W> Pv[U], Mv[U];
#pragma unroll
  for (int v = 0; v < U; ++v) {
    Pv[v] = ~(EditWord<W>)0;
    Mv[v] = 0;
  }
  uint32_t left = m_b;
  for (uint32_t w = 0; w < rw; ++w) {
    uint32_t codes[U];  // (scalar: every lane reads the same word)
#pragma unroll
    for (int v = 0; v < U; ++v) codes[v] = __builtin_amdgcn_readfirstlane(rec[v * rw + w]);
    const uint32_t cols = left < kCols ? left : kCols;
    left -= cols;
    for (uint32_t c = 0; c < cols; ++c) {
#pragma unroll
      for (int v = 0; v < U; ++v) {
        edit_column<W>(edit_eq<P, W, IUPAC>(a, codes[v]), Pv[v], Mv[v]);
        codes[v] >>= P;
      }
    }
  }
#pragma unroll
  for (int v = 0; v < U; ++v) cost[v] = edit_score<W>(Pv[v], Mv[v], rows, m_b);
}

// records a lane steps side by side: what keeps the vector unit supplied with independent work and lets a round's scalar
// work and its one branch be shared, against the registers of U pairs of bit vectors
template <int W>
constexpr int edit_unroll() { return W == 1 ? 4 : 2; }

// The walk of one lane over the targets of chunk c, shared by the survey and the fill: hit(r, j, strand, cost) for every
// candidate the call visits, in ascending r.  Lanes beyond n_a walk along and never hit.  The whole workgroup calls it (it
// stages the tiles together); a wavefront with wave_active == false only helps staging.
template <int P, int W, bool IUPAC, typename Hit>
__device__ __forceinline__ void edit_walk(const EditArgs& A, uint64_t i, bool valid, bool wave_active, uint64_t c, const EditWord<W> (&a)[P], Hit&& hit) {
  constexpr int U = edit_unroll<W>();
  __shared__ uint32_t tile[kEditTileWords];
  const uint32_t rw = A.rw, T = kEditTileWords / rw;  // words per record, records per tile
  const uint64_t ib = (uint64_t)blockIdx.x * kPairsStrip;
  const uint64_t i0 = ib + (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(threadIdx.x / kWave)) * kPairsWave;
  const uint64_t j0 = pairs_chunk_begin(A.chunk, c), j1 = pairs_chunk_end(A.chunk, A.n_b, c);
  const uint32_t S = A.S, m_b = A.m_b, k = A.k, mode = A.mode;
  const EditWord<W> rows = edit_rows<W>(A.m_a);
  // the first record of the workgroup's walk and of this wavefront's: a self-mode tile starts at its own first entry
  const uint64_t r_group = pairs_tile_first(mode, ib, j0, j1) * S, r_wave = pairs_tile_first(mode, i0, j0, j1) * S;
  const uint64_t r_end = j1 * S;
  auto candidate = [&](uint32_t r, uint32_t cost) {
    const uint32_t strand = S == 2 ? (r & 1u) : 0u;
    const uint64_t j = S == 2 ? (r >> 1) : r;
    if (valid && cost <= k && pairs_visits(mode, i, j, strand)) hit(r, j, strand, cost);
  };
  for (uint64_t rt = r_group; rt < r_end; rt += T) {
    const uint32_t cnt = r_end - rt < (uint64_t)T ? (uint32_t)(r_end - rt) : T;
    __syncthreads();  // (the tile before this one has been read)
    uint32_t stage[kEditTileWords / kPairsStrip];
#pragma unroll
    for (uint32_t e = 0; e < kEditTileWords / kPairsStrip; ++e) {
      const uint32_t q = threadIdx.x + e * kPairsStrip;
      stage[e] = q < cnt * rw ? A.t[(size_t)rt * rw + q] : 0u;
    }
#pragma unroll
    for (uint32_t e = 0; e < kEditTileWords / kPairsStrip; ++e) tile[threadIdx.x + e * kPairsStrip] = stage[e];
    __syncthreads();
    if (!wave_active) continue;
    uint32_t u = r_wave <= rt ? 0u : r_wave - rt < cnt ? (uint32_t)(r_wave - rt) : cnt;
    for (; u + U <= cnt; u += U) {
      uint32_t cost[U];
      edit_round<P, W, IUPAC, U>(a, tile + u * rw, rw, m_b, rows, cost);
      uint32_t least = cost[0];
#pragma unroll
      for (int v = 1; v < U; ++v) least = cost[v] < least ? cost[v] : least;
      if (__ballot(least <= k) != 0ull) {  // rare
#pragma unroll
        for (int v = 0; v < U; ++v) candidate((uint32_t)(rt + u + v), cost[v]);
      }
    }
    for (; u < cnt; ++u) {  // (the last records of a chunk)
      uint32_t cost[1];
      edit_round<P, W, IUPAC, 1>(a, tile + u * rw, rw, m_b, rows, cost);
      if (__ballot(cost[0] <= k) != 0ull) candidate((uint32_t)(rt + u), cost[0]);
    }
  }
}

template <int P, int W>
__device__ __forceinline__ void edit_load_entry(const EditArgs& A, uint64_t i, bool valid, EditWord<W> (&a)[P]) {
  uint32_t planes[P * W];
#pragma unroll
  for (int q = 0; q < P * W; ++q) planes[q] = valid ? A.a[(size_t)i * (P * W) + q] : 0u;
  edit_entry_planes<P, W>(planes, a);
}

template <int P, int W, bool IUPAC>
__global__ __launch_bounds__(kPairsStrip) void edit_survey_kernel(EditArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * kPairsStrip + threadIdx.x;
  const uint64_t c = blockIdx.y;
  const bool valid = i < A.n_a;
  EditWord<W> a[P];
  edit_load_entry<P, W>(A, i, valid, a);
  PairsCell cell = pairs_empty_cell();
  edit_walk<P, W, IUPAC>(A, i, valid, true, c, a, [&](uint32_t r, uint64_t, uint32_t, uint32_t cost) { cell = pairs_combine(cell, PairsCell{cost, r, 1u, 1u}); });
  if (valid) A.cells[c * A.n_a + i] = make_uint4(cell.cost, cell.r, cell.ties, cell.n_hits);
}

template <int P, int W, bool IUPAC>
__global__ __launch_bounds__(kPairsStrip) void edit_fill_kernel(EditArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * kPairsStrip + threadIdx.x;
  const uint64_t c = blockIdx.y;
  const bool valid = i < A.n_a;
  uint4 cell = make_uint4(0, 0, 0, 0);
  if (valid) cell = A.cells[c * A.n_a + i];
  const bool wave_active = __ballot(cell.w != 0u) != 0ull;  // (else: the tile holds no candidate)
  if (!__syncthreads_or(wave_active)) return;               // no tile of the strip does: nothing to stage
  EditWord<W> a[P];
  edit_load_entry<P, W>(A, i, valid, a);
  uint64_t pos = valid ? A.row_first[i] + cell.z : 0;  // (cell.z: the place in the row, pairs_rows_kernel)
  edit_walk<P, W, IUPAC>(A, i, valid, wave_active, c, a, [&](uint32_t, uint64_t j, uint32_t strand, uint32_t cost) {
    sassy_hip_EditPair rec;
    rec.a_idx = (uint32_t)i; rec.b_idx = (uint32_t)j; rec.cost = (uint8_t)cost; rec.strand = (uint8_t)strand; rec.pad_[0] = rec.pad_[1] = 0;
    A.out[pos++] = rec;
  });
}

// edit_clusters: the survey's walk over the self-mode triangle with a union step in place of the cell (cluster_step.h).  j is
// the same for the whole wavefront, so the look at parent[j] that comes first is one broadcast load; a lane whose register
// already names j's parent goes on without a chase or a write.
template <int P, int W, bool IUPAC>
__global__ __launch_bounds__(kPairsStrip) void edit_cluster_kernel(EditArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * kPairsStrip + threadIdx.x;
  const uint64_t c = blockIdx.y;
  const bool valid = i < A.n_a;
  EditWord<W> a[P];
  edit_load_entry<P, W>(A, i, valid, a);
  ClusterDeviceMem mem{A.parent};
  uint32_t root = (uint32_t)i;
  edit_walk<P, W, IUPAC>(A, i, valid, true, c, a, [&](uint32_t, uint64_t j, uint32_t, uint32_t) {
    if (j != i) cluster_join(mem, (uint32_t)i, (uint32_t)j, root);  // ((i, i, 1) is no edge)
  });
}

// which kernel walks: the survey, the fill pass of edit_pairs, the link pass of edit_clusters
enum : int { kWalkSurvey = 0, kWalkFill = 1, kWalkCluster = 2 };
template <int P, bool IUPAC>
hipError_t launch_walk(int kind, uint32_t W, const EditArgs& A, dim3 grid, hipStream_t st) {
  if (W == 1) {
    if (kind == kWalkCluster) hipLaunchKernelGGL((edit_cluster_kernel<P, 1, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
    else if (kind == kWalkFill) hipLaunchKernelGGL((edit_fill_kernel<P, 1, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
    else hipLaunchKernelGGL((edit_survey_kernel<P, 1, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
  } else {
    if (kind == kWalkCluster) hipLaunchKernelGGL((edit_cluster_kernel<P, 2, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
    else if (kind == kWalkFill) hipLaunchKernelGGL((edit_fill_kernel<P, 2, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
    else hipLaunchKernelGGL((edit_survey_kernel<P, 2, IUPAC>), grid, dim3(kPairsStrip), 0, st, A);
  }
  return hipGetLastError();
}
hipError_t launch_walk_profile(Profile pr, int kind, uint32_t W, const EditArgs& A, dim3 grid, hipStream_t st) {
  if (pr == PROFILE_DNA) return launch_walk<2, false>(kind, W, A, grid, st);
  if (pr == PROFILE_IUPAC) return launch_walk<4, true>(kind, W, A, grid, st);
  return launch_walk<8, false>(kind, W, A, grid, st);
}

// A call behind its refusals: the plan, the walk's arguments, its grid.
struct EditRun {
  PairsPlan plan;
  EditArgs args{};
  uint32_t W = 1;
  dim3 grid;
};
// The first half of a call behind its refusals: the plan, both lists encoded and uploaded, the walk's arguments and grid, the
// stats' geometry.  want_cells: the partials matrix too (the clustering walk has none).
int edit_stage(sassy_SearcherType* s, const uint8_t* a, size_t n_a, uint32_t m_a, const uint8_t* b, size_t n_b, uint32_t m_b, uint32_t k, uint32_t self_mode,
               bool want_cells, EditRun& R) {
  hipStream_t st = s->stream;
  const bool self = b == nullptr;
  const uint32_t S = s->rc ? 2u : 1u, P = pairs_planes(s->profile), W = pairs_words(m_a), PW = P * W, rw = edit_record_words(P, m_b);
  const size_t nb = self ? n_a : n_b;
  const uint8_t* targets = self ? a : b;
  R.W = W;
  R.plan = pairs_plan(n_a, nb, self ? self_mode : kPairsCross, s->sw.pairs_chunks, self_mode == kPairsSelfPairs ? kEditFineChunk : 0);
  std::vector<uint32_t> ha(n_a * PW), ht(nb * S * rw);
  pairs_for_slices(n_a, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) pairs_encode(s->profile, a + i * m_a, m_a, W, ha.data() + i * PW);
  });
  pairs_for_slices(nb, [&](size_t j0, size_t j1) {
    uint8_t rev[kEditMaxRows];
    for (size_t j = j0; j < j1; ++j) {
      edit_encode_record(s->profile, targets + j * m_b, m_b, ht.data() + j * S * rw);
      if (S == 2) {
        pairs_reverse_complement(targets + j * m_b, m_b, [&](uint8_t c) { return complement_char(s->profile, c); }, rev);
        edit_encode_record(s->profile, rev, m_b, ht.data() + (j * S + 1) * rw);
      }
    }
  });
  if (int rc = s->d_pairs_a.reserve(ha.size())) return rc;
  if (int rc = s->d_pairs_t.reserve(ht.size())) return rc;
  if (want_cells)
    if (int rc = s->d_pairs_cells.reserve((size_t)R.plan.n_chunks * n_a)) return rc;
  HIP_TRY(hipMemcpyAsync(s->d_pairs_a.p, ha.data(), ha.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(s->d_pairs_t.p, ht.data(), ht.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));  // (the host vectors go away)
  EditArgs& A = R.args;
  A.a = s->d_pairs_a.p; A.t = s->d_pairs_t.p;
  A.n_a = n_a; A.n_b = nb; A.chunk = R.plan.chunk;
  A.S = S; A.m_a = m_a; A.m_b = m_b; A.rw = rw; A.k = k; A.mode = R.plan.mode;
  A.cells = want_cells ? s->d_pairs_cells.p : nullptr;
  R.grid = dim3((uint32_t)R.plan.n_strips, R.plan.n_chunks);
  s->stats.scan_launches = 1;
  s->stats.chunks = R.plan.n_chunks;
  s->stats.grid = (uint32_t)R.plan.n_strips;
  s->stats.blocks_per_chunk = (uint32_t)std::min<uint64_t>(R.plan.chunk, 0xFFFFFFFFull);
  s->stats.text_bytes = (uint64_t)n_a * m_a + (uint64_t)nb * m_b;
  return 0;
}
// The survey: the partials matrix filled.
int edit_survey(sassy_SearcherType* s, const uint8_t* a, size_t n_a, uint32_t m_a, const uint8_t* b, size_t n_b, uint32_t m_b, uint32_t k, uint32_t self_mode,
                EditRun& R) {
  hipStream_t st = s->stream;
  if (int rc = edit_stage(s, a, n_a, m_a, b, n_b, m_b, k, self_mode, true, R)) return rc;
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[0], st));
  HIP_TRY(launch_walk_profile(s->profile, kWalkSurvey, R.W, R.args, R.grid, st));
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[1], st));
  return 0;
}
// E >= |m_a - m_b|: beyond k no pair is a candidate and nothing is launched
bool edit_lengths_too_far(size_t m_a, size_t m_b, size_t k) { return (m_a > m_b ? m_a - m_b : m_b - m_a) > k; }

}  // namespace

// What both entry points refuse, before any device work; self: b == NULL && n_b == 0, where m_b is 0 or m_a.
int edit_refusals(sassy_SearcherType* s, bool have_out, const uint8_t* a, size_t n_a, size_t m_a, const uint8_t* b, size_t n_b, size_t m_b, size_t k,
                  uint32_t flags, const char* who) {
  const std::string w(who);
  if (!s || !a || !have_out) return fail(SASSY_HIP_EINVAL, "Pointers in " + w + "() must not be null");
  if (flags) return fail(SASSY_HIP_EINVAL, w + " takes no flags (the sequences are host bytes)");
  if (m_a == 0) return fail(SASSY_HIP_EINVAL, w + ": m_a must be at least 1");
  if (m_a > kEditMaxRows) return fail(SASSY_HIP_EINVAL, w + ": m_a must be <= " + std::to_string(kEditMaxRows) + " (got " + std::to_string(m_a) + ")");
  if (k > 254) return fail(SASSY_HIP_EINVAL, w + ": k must be <= 254 (the pair records' costs are bytes)");
  if (n_a == 0) return fail(SASSY_HIP_EINVAL, w + " needs at least one sequence in a");
  if (b && n_b == 0) return fail(SASSY_HIP_EINVAL, w + ": b is given but n_b is 0 (self mode is b == NULL and n_b == 0)");
  if (!b && n_b) return fail(SASSY_HIP_EINVAL, w + ": b is NULL but n_b is " + std::to_string(n_b));
  if (!b && m_b != 0 && m_b != m_a)
    return fail(SASSY_HIP_EINVAL, w + ": self mode compares a with itself, m_b must be 0 or m_a (got " + std::to_string(m_b) + ", m_a is " + std::to_string(m_a) + ")");
  if (b && m_b == 0) return fail(SASSY_HIP_EINVAL, w + ": m_b must be at least 1");
  if (m_b > kEditMaxRows) return fail(SASSY_HIP_EINVAL, w + ": m_b must be <= " + std::to_string(kEditMaxRows) + " (got " + std::to_string(m_b) + ")");
  if (n_a > 0x7FFFFFFFull || n_b > 0x7FFFFFFFull)
    return fail(SASSY_HIP_EUNSUPPORTED, w + " takes at most 2^31 - 1 sequences per list (" + std::to_string(std::max(n_a, n_b)) + ")");
  if (!std::isnan(s->max_n_frac)) return fail(SASSY_HIP_EUNSUPPORTED, w + " does not take max_n_frac: there is no text span for it to apply to");
  // the family's own checks, on each list as it stands: the sequences are its patterns, so "pattern N" in its messages is
  // sequence N of the list named behind the message
  auto family = [&](const uint8_t* list, size_t n, size_t m, const char* name) {
    std::vector<const uint8_t*> seqs(n);
    for (size_t i = 0; i < n; ++i) seqs[i] = list + i * m;
    const std::vector<size_t> lens(n, m);
    const int rc = hamming_refusals(s, seqs.data(), lens.data(), n, k, who);
    if (rc) g_err += std::string(" (") + who + ": list " + name + ")";
    return rc;
  };
  if (int rc = family(a, n_a, m_a, "a")) return rc;
  return b ? family(b, n_b, m_b, "b") : 0;
}

// edit_clusters (clusters.hip): the list staged as a self-mode pairs call stages it, one launch of the link kernel
int edit_link_components(sassy_SearcherType* s, const uint8_t* a, size_t n, uint32_t m, uint32_t k, uint32_t* d_parent) {
  hipStream_t st = s->stream;
  EditRun R;
  if (int rc = edit_stage(s, a, n, m, nullptr, 0, m, k, kPairsSelfPairs, false, R)) return rc;
  R.args.parent = d_parent;
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[0], st));
  HIP_TRY(launch_walk_profile(s->profile, kWalkCluster, R.W, R.args, R.grid, st));
  if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[1], st));
  return 0;
}

}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_edit_pairs(sassy_SearcherType* s, const uint8_t* a, size_t n_a, size_t m_a, const uint8_t* b, size_t n_b, size_t m_b, size_t k, uint32_t flags,
                         sassy_hip_EditPair** out, size_t* n_out) {
  const char* who = "edit_pairs";
  return pairs_guarded(who, [&]() -> int {
  if (int rc = edit_refusals(s, out && n_out, a, n_a, m_a, b, n_b, m_b, k, flags, who)) return rc;
  *out = nullptr;
  *n_out = 0;
  if (!b) m_b = m_a;
  const size_t lens[2] = {m_a, m_b};
  return hamming_call(s, lens, 2, k, [&](uint32_t kk) {  // (k >= the longer length: every pair is a record)
    s->stats.filtered = 9;
    if (edit_lengths_too_far(m_a, m_b, kk)) return 0;
    hipStream_t st = s->stream;
    EditRun R;
    if (int rc = edit_survey(s, a, n_a, (uint32_t)m_a, b, n_b, (uint32_t)m_b, kk, kPairsSelfPairs, R)) return rc;
    const unsigned long long* row_first = nullptr;
    unsigned long long total = 0;
    if (int rc = pairs_place_rows(s, R.args.cells, n_a, R.plan.n_chunks, &row_first, &total)) return rc;
    if (total > 0xFFFFFFFFull) return fail(SASSY_HIP_ENOMEM, "edit_pairs: more than 2^32 - 1 records (" + std::to_string(total) + ")");
    if (total == 0) {
      pairs_times(s, false);
      return 0;
    }
    if (int rc = s->d_pairs_out.reserve((size_t)total * sizeof(sassy_hip_EditPair))) return rc;
    R.args.row_first = row_first;
    R.args.out = reinterpret_cast<sassy_hip_EditPair*>(s->d_pairs_out.p);
    HIP_TRY(launch_walk_profile(s->profile, kWalkFill, R.W, R.args, R.grid, st));
    if (s->timing >= 2) HIP_TRY(hipEventRecord(s->ev_line[3], st));
    s->stats.scan_launches = 2;
    return pairs_take_records(s, total, out, n_out);
  });
  });
}

void sassy_hip_edit_pairs_free(sassy_hip_EditPair* p) { free(p); }

int sassy_hip_edit_nearest(sassy_SearcherType* s, const uint8_t* a, size_t n_a, size_t m_a, const uint8_t* b, size_t n_b, size_t m_b, size_t k, uint32_t flags,
                           uint8_t* out_cost, uint32_t* out_index, uint8_t* out_strand, uint32_t* out_ties) {
  const char* who = "edit_nearest";
  return pairs_guarded(who, [&]() -> int {
  if (int rc = edit_refusals(s, out_cost != nullptr, a, n_a, m_a, b, n_b, m_b, k, flags, who)) return rc;
  if (!b) m_b = m_a;
  const size_t lens[2] = {m_a, m_b};
  return hamming_call(s, lens, 2, k, [&](uint32_t kk) {
    s->stats.filtered = 9;
    if (edit_lengths_too_far(m_a, m_b, kk)) {  // no entry has a candidate
      memset(out_cost, SASSY_HIP_NO_MATCH, n_a);
      if (out_index) memset(out_index, 0xFF, n_a * 4);
      if (out_strand) memset(out_strand, 0, n_a);
      if (out_ties) memset(out_ties, 0, n_a * 4);
      return 0;
    }
    EditRun R;
    if (int rc = edit_survey(s, a, n_a, (uint32_t)m_a, b, n_b, (uint32_t)m_b, kk, kPairsSelfNearest, R)) return rc;
    return pairs_fold_nearest(s, R.args.cells, n_a, R.plan.n_chunks, R.args.S, out_cost, out_index, out_strand, out_ties);
  });
  });
}

}  // extern "C"
