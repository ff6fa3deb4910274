// dedup_reads.hip -- UMI grouping and deduplication of a resident read batch (sassy_hip_umi_groups_reads,
// sassy_hip_dedup_reads): the key of a read is a window at one of its ends, the groups are what
// sassy_hip_umi_groups makes of the windows, and of every group the read with the highest score is kept, as a NEW resident read
// batch.  The arithmetic -- the refusals, the window's planes, the reverse complement, the score and its key -- is
// dedup_step.h's; the window is demux_step.h's; a block of a window is trim_step.h's; the grouping behind the upload is
// umi_groups.hip's (umi_groups_resident); the scan is the pair family's (pairs_scan_u64); the layout rule and its scan are the
// parse's (reads_layout_windows); the write kernel is the trim's (write_windows).
//
// Device work, all on the searcher's stream:
//   dedup_flag_kernel     a lane per read: has_window[r]
//   pairs_scan_u64        the reads that have a window, numbered in ascending order; the total -> host (one wait)
//   dedup_encode_kernel<P, IUPAC, RC>   a lane per read: the window through trm_window_block (one block for m <= 64, two for m <= 128), its
//              bytes into pairs_encode's planes at d_pairs_a[idx]; an rc searcher: both strands of the target record at
//              d_pairs_t[2 idx], [2 idx + 1]; src[idx] = r
//   umi_groups_resident   collapse, scan, gather, walk, relaxation, expand over the compacted arrays
//   dedup_scatter_kernel  a lane per read: the four columns mapped back through src, the sentinels where there is no window
//   -- sassy_hip_dedup_reads only --
//   dedup_score_kernel    eight lanes per read: the sum of its quality bytes by 16-byte loads (its length where the handle keeps
//              none), one 64-bit atomic max into best[label[r]]
//   dedup_keep_kernel     a lane per read: is its key its group's best?
//   pairs_scan_u64        the kept reads numbered; the total -> host (one wait)
//   dedup_compact_kernel  the kept reads' table and lengths
//   fastq_rec_sum / _top / _write_kernel, reads_window_write_kernel<false, true>    the new handle, as reads_select makes it
// The input handle is only read.  Every load of a read's bytes is bounded by the handle's length table and its text size, every
// store by the read count or by the count of the scan that numbered it.
#include <hip/hip_runtime.h>

#include "host_internal.h"
#include "dedup_step.h"

static_assert(SASSY_HIP_DEDUP_END3 == sassy_hip::kDdpEnd3 && SASSY_HIP_UMI_DIRECTIONAL == sassy_hip::kDdpMaxMethod &&
                  sassy_hip::kDdpMaxLen == sassy_hip::kPairsMaxRows,
              "the header's numbers are the step header's");

namespace sassy_hip {
namespace {

struct ReadTable {
  const uint64_t *start, *len;  // the handle's tables
  uint64_t bytes;               // the handle's text size
  uint64_t n;
  uint32_t at, m, end3;
};
// the read's first byte and its length as the kernels take it (reads_fit_len)
__device__ __forceinline__ uint32_t table_len(const ReadTable& T, uint64_t r, uint64_t* s0) {
  *s0 = T.start[r];
  return reads_fit_len(*s0, T.len[r], T.bytes, kOvlMaxLen);
}

__global__ __launch_bounds__(256) void dedup_flag_kernel(ReadTable T, unsigned long long* has_window) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= T.n) return;
  uint64_t s0;
  has_window[r] = dmx_has_window(table_len(T, r, &s0), T.at, T.m) ? 1ull : 0ull;
}

struct EncodeArgs {
  ReadTable T;
  const uint8_t* text;
  const unsigned long long *has_window, *dense;
  uint64_t n_w;         // reads with a window: the entries of the arrays below
  uint32_t W;           // words per plane as stored
  uint32_t *a, *t;      // [n_w][P W], [2 n_w][P W] (RC: both strands of the target records)
  uint32_t* src;        // [n_w]
};
template <int P, bool IUPAC, bool RC>
__global__ __launch_bounds__(256) void dedup_encode_kernel(EncodeArgs A) {
  constexpr uint32_t profile = IUPAC ? kHamIupac : kHamDna;
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= A.T.n || !A.has_window[r]) return;
  const uint64_t idx = A.dense[r];
  if (idx >= A.n_w) return;  // (never: the scan numbered exactly n_w reads)
  uint64_t s0;
  const uint32_t la = table_len(A.T, r, &s0);
  const TrmLoad16 load16{A.text};
  const uint64_t at = s0 + dmx_window(la, A.T.at, A.T.m, A.T.end3 != 0u);
  const uint32_t W = A.W, PW = P * W;
  uint32_t fw[P][4], rv[P][4];
  ddp_window_planes<P, RC>(profile, load16, at, A.T.bytes, A.T.m, fw, rv);
  uint32_t* a = A.a + idx * PW;
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int w = 0; w < 4; ++w)
      if ((uint32_t)w < W) a[p * W + w] = fw[p][w];
  if (RC) {
    uint32_t *t0 = A.t + 2 * idx * PW, *t1 = t0 + PW;
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if ((uint32_t)w < W) {
          t0[p * W + w] = fw[p][w];
          t1[p * W + w] = rv[p][w];
        }
  }
  A.src[idx] = (uint32_t)r;
}

struct ScatterArgs {
  uint64_t n, n_w;
  const unsigned long long *has_window, *dense;
  const uint32_t* src;
  UmiColumns in;  // n_w entries each, indices into the compacted list
  uint32_t *label, *size, *rep, *count;  // n entries each
};
__global__ __launch_bounds__(256) void dedup_scatter_kernel(ScatterArgs A) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= A.n) return;
  uint32_t label = kDdpNone, rep = kDdpNone, size = 0, count = 0;
  const uint64_t j = A.dense[r];
  if (A.has_window[r] && j < A.n_w) {
    const uint32_t jl = A.in.label[j], jr = A.in.rep[j];
    label = jl < A.n_w ? A.src[jl] : kDdpNone;  // (always below: indices of the list)
    rep = jr < A.n_w ? A.src[jr] : kDdpNone;
    size = A.in.size[j];
    count = A.in.count[j];
  }
  A.label[r] = label; A.size[r] = size; A.rep[r] = rep; A.count[r] = count;
}

struct ScoreArgs {
  ReadTable T;
  const uint8_t* qual;  // NULL: the score is the length
  const uint32_t* label;
  unsigned long long *key, *best;  // [n]: the read's key (0: no window); the best key of the group that read r labels
};
// kDdpScoreLanes lanes share a read and load neighbouring 16-byte pieces of it: 128 contiguous bytes a step, 32 reads a
// workgroup.  Every lane stays to the end (the sums meet in a shuffle).
template <bool QUAL>
__global__ __launch_bounds__(256) void dedup_score_kernel(ScoreArgs A) {
  const uint64_t thread = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t r = thread / kDdpScoreLanes;
  const uint32_t q = (uint32_t)(thread % kDdpScoreLanes);
  const bool live = r < A.T.n;
  uint64_t s0 = 0;
  const uint32_t la = live ? table_len(A.T, r, &s0) : 0u;
  uint32_t sum = 0;
  if (QUAL) {
    const uint32_t pieces = ddp_pieces(la);
    for (uint32_t piece = q; piece < pieces; piece += kDdpScoreLanes) {  // (16 piece < la <= bytes - s0)
      const uint4 v = *reinterpret_cast<const uint4*>(A.qual + s0 + 16u * piece);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      sum += ddp_piece_sum(w, piece, la);
    }
#pragma unroll
    for (uint32_t o = 1; o < kDdpScoreLanes; o <<= 1) sum += __shfl_xor(sum, (int)o);
  } else {
    sum = la;
  }
  if (!live || q != 0) return;
  const uint32_t label = A.label[r];
  const bool grouped = label != kDdpNone && label < A.T.n;
  const uint64_t key = grouped ? ddp_key(sum, (uint32_t)r) : 0ull;
  A.key[r] = key;
  if (grouped) (void)__hip_atomic_fetch_max(A.best + label, (unsigned long long)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void dedup_keep_kernel(uint64_t n, const uint32_t* label, const unsigned long long* key, const unsigned long long* best,
                                                         unsigned long long* keep) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const uint32_t l = label[r];
  keep[r] = (l != kDdpNone && l < n && key[r] != 0ull && best[l] == key[r]) ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void dedup_compact_kernel(uint64_t n, uint64_t n_kept, const unsigned long long* keep, const unsigned long long* dense,
                                                            const uint64_t* len, uint64_t* kept_src, uint64_t* kept_len) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n || !keep[r]) return;
  const uint64_t j = dense[r];
  if (j >= n_kept) return;  // (never: the scan numbered exactly n_kept reads)
  kept_src[j] = r;
  kept_len[j] = len[r];
}

// what a refusal of the calls' own checks says
std::string refusal_text(DdpRefusal why, const DdpCall& c, const std::string& who) {
  if (why == kDdpNullSearcher) return "Pointers in " + who + "() must not be null";
  if (why == kDdpFlags) return who + " takes SASSY_HIP_DEDUP_END3 only (the read batch is on the device)";
  if (why == kDdpMethod) return who + ": unknown method " + std::to_string(c.method) + " (0 unique, 1 cluster, 2 directional)";
  if (why == kDdpLen) return who + ": m must be 1 .. " + std::to_string(kDdpMaxLen) + " (got " + std::to_string(c.m) + ")";
  if (why == kDdpAt)
    return who + ": at + m = " + std::to_string((uint64_t)c.at + c.m) + " reaches past the longest read a batch may hold (" + std::to_string(kOvlMaxLen) + ")";
  if (why == kDdpNullOut) return "Pointers in " + who + "() must not be null (" + (who == "dedup_reads" ? "out_dedup" : "out_label") + ")";
  return who + ": refused";
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct DdpOut {
  uint32_t *label, *size, *rep, *count;  // host, n each; any may be NULL
  uint64_t* kept;                        // host, n; may be NULL
  size_t *n_unique, *n_groups;           // may be NULL
};

// The calls behind their refusals, inside reads_new_batch (the device, fresh stats, k cut to m).  F: the fresh handle where the
// kept reads are wanted, NULL for the groups alone.
int dedup_run(sassy_SearcherType* s, const sassy_hip_Reads* reads, uint32_t at, uint32_t m, uint32_t k, uint32_t method, uint32_t flags, const DdpOut& O,
              sassy_hip_Reads* F, const char* who) {
  hipStream_t st = s->stream;
  const uint64_t n = reads->n_records;
  const bool keep_quality = reads->d_qual != nullptr;
  if (O.n_unique) *O.n_unique = 0;
  if (O.n_groups) *O.n_groups = 0;
  // no read, or none that is long enough for a window (the longest is not): no kernel
  if (n == 0 || reads->longest < (uint64_t)at + m) {
    for (uint64_t r = 0; r < n; ++r) {
      if (O.label) O.label[r] = kDdpNone;
      if (O.rep) O.rep[r] = kDdpNone;
      if (O.size) O.size[r] = 0;
      if (O.count) O.count[r] = 0;
    }
    if (F) {
      if (int rc = reads_empty_buffers(F, keep_quality, st)) return rc;
      HIP_TRY(hipStreamSynchronize(st));
    }
    s->stats.filtered = 12;
    return 0;
  }
  if (n > 0x7FFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, std::string(who) + " takes at most 2^31 - 1 reads (" + std::to_string(n) + ")");
  // the flag kernel, the scan's three, the encode kernel, the scatter kernel; the Dna look where it runs; below, the walk's own
  uint32_t launches = 6;
  if (int rc = reads_require_plain(s, reads, who, "the reads hold", "encode", &launches)) return rc;

  // one area: the flags and their scan (used twice: the windows, then the kept reads), the block sums, the reads' table, the four
  // columns, the keys, the groups' best keys, the kept reads' table and lengths
  const size_t n_blocks = pairs_scan_blocks(n);
  const size_t o_flag = 0, o_dense = o_flag + up256(n * 8), o_sums = o_dense + up256(n * 8), o_src = o_sums + up256((n_blocks + 1) * 8),
               o_label = o_src + up256(n * 4), o_size = o_label + up256(n * 4), o_rep = o_size + up256(n * 4), o_count = o_rep + up256(n * 4),
               o_key = o_count + up256(n * 4), o_best = o_key + up256(F ? n * 8 : 0), o_ksrc = o_best + up256(F ? n * 8 : 0),
               o_klen = o_ksrc + up256(F ? n * 8 : 0), total = o_klen + up256(F ? n * 8 : 0);
  if (int rc = s->d_dedup.reserve(total)) return rc;
  uint8_t* base = s->d_dedup.p;
  unsigned long long *d_flag = reinterpret_cast<unsigned long long*>(base + o_flag), *d_dense = reinterpret_cast<unsigned long long*>(base + o_dense),
                     *d_sums = reinterpret_cast<unsigned long long*>(base + o_sums), *d_key = reinterpret_cast<unsigned long long*>(base + o_key),
                     *d_best = reinterpret_cast<unsigned long long*>(base + o_best);
  uint32_t *d_src = reinterpret_cast<uint32_t*>(base + o_src), *d_label = reinterpret_cast<uint32_t*>(base + o_label),
           *d_size = reinterpret_cast<uint32_t*>(base + o_size), *d_rep = reinterpret_cast<uint32_t*>(base + o_rep),
           *d_count = reinterpret_cast<uint32_t*>(base + o_count);
  uint64_t *d_ksrc = reinterpret_cast<uint64_t*>(base + o_ksrc), *d_klen = reinterpret_cast<uint64_t*>(base + o_klen);

  ReadTable T{reads->d_table, reads->d_table + n, reads->text_bytes, n, at, m, (flags & kDdpEnd3) ? 1u : 0u};
  const dim3 per_read((uint32_t)((n + 255) / 256)), block(256);
  hipLaunchKernelGGL(dedup_flag_kernel, per_read, block, 0, st, T, d_flag);
  HIP_TRY(hipGetLastError());
  if (int rc = pairs_scan_u64(s, d_flag, n, d_sums, d_dense)) return rc;
  unsigned long long n_w = 0;
  HIP_TRY(hipMemcpyAsync(&n_w, d_sums + n_blocks, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (n_w == 0 || n_w > n) return fail(SASSY_HIP_EINVAL, std::string(who) + ": the handle's longest read has no window after all (internal error)");

  const uint32_t P = pairs_planes(s->profile), W = pairs_words(m), PW = P * W;
  if (int rc = s->d_pairs_a.reserve((size_t)n_w * PW)) return rc;
  if (s->rc)
    if (int rc = s->d_pairs_t.reserve((size_t)n_w * 2 * PW)) return rc;
  EncodeArgs E;
  E.T = T;
  E.text = reads->d_text;
  E.has_window = d_flag; E.dense = d_dense;
  E.n_w = n_w;
  E.W = W;
  E.a = s->d_pairs_a.p; E.t = s->rc ? s->d_pairs_t.p : nullptr;
  E.src = d_src;
  if (s->profile == PROFILE_IUPAC) {
    if (s->rc) hipLaunchKernelGGL((dedup_encode_kernel<4, true, true>), per_read, block, 0, st, E);
    else hipLaunchKernelGGL((dedup_encode_kernel<4, true, false>), per_read, block, 0, st, E);
  } else {
    if (s->rc) hipLaunchKernelGGL((dedup_encode_kernel<2, false, true>), per_read, block, 0, st, E);
    else hipLaunchKernelGGL((dedup_encode_kernel<2, false, false>), per_read, block, 0, st, E);
  }
  HIP_TRY(hipGetLastError());

  UmiColumns cols{};
  size_t n_unique = 0;
  if (int rc = umi_groups_resident(s, E.a, s->rc ? E.t : E.a, (size_t)n_w, m, k, method, nullptr, nullptr, nullptr, nullptr, &n_unique, nullptr, &cols))
    return rc;
  const uint32_t walk_launches = s->stats.scan_launches;

  ScatterArgs Sc{n, n_w, d_flag, d_dense, d_src, cols, d_label, d_size, d_rep, d_count};
  hipLaunchKernelGGL(dedup_scatter_kernel, per_read, block, 0, st, Sc);
  HIP_TRY(hipGetLastError());
  if (O.label) HIP_TRY(hipMemcpyAsync(O.label, d_label, n * 4, hipMemcpyDeviceToHost, st));
  if (O.size) HIP_TRY(hipMemcpyAsync(O.size, d_size, n * 4, hipMemcpyDeviceToHost, st));
  if (O.rep) HIP_TRY(hipMemcpyAsync(O.rep, d_rep, n * 4, hipMemcpyDeviceToHost, st));
  if (O.count) HIP_TRY(hipMemcpyAsync(O.count, d_count, n * 4, hipMemcpyDeviceToHost, st));
  launches += walk_launches;
  size_t n_groups = 0;

  if (!F) {
    HIP_TRY(hipStreamSynchronize(st));
    for (uint64_t r = 0; r < n; ++r) n_groups += O.label[r] == r;  // (out_label is required here)
  } else {
    HIP_TRY(hipMemsetAsync(d_best, 0, n * 8, st));
    ScoreArgs Sa{T, reads->d_qual, d_label, d_key, d_best};
    const dim3 score_grid((uint32_t)((n * kDdpScoreLanes + 255) / 256));
    if (keep_quality) hipLaunchKernelGGL(dedup_score_kernel<true>, score_grid, block, 0, st, Sa);
    else hipLaunchKernelGGL(dedup_score_kernel<false>, score_grid, block, 0, st, Sa);
    hipLaunchKernelGGL(dedup_keep_kernel, per_read, block, 0, st, n, (const uint32_t*)d_label, (const unsigned long long*)d_key,
                       (const unsigned long long*)d_best, d_flag);
    HIP_TRY(hipGetLastError());
    if (int rc = pairs_scan_u64(s, d_flag, n, d_sums, d_dense)) return rc;
    unsigned long long n_kept = 0;
    HIP_TRY(hipMemcpyAsync(&n_kept, d_sums + n_blocks, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_kept == 0 || n_kept > n_w) return fail(SASSY_HIP_EINVAL, std::string(who) + ": a group lost its best read (internal error)");
    hipLaunchKernelGGL(dedup_compact_kernel, per_read, block, 0, st, n, (uint64_t)n_kept, (const unsigned long long*)d_flag,
                       (const unsigned long long*)d_dense, reads->d_table + n, d_ksrc, d_klen);
    HIP_TRY(hipGetLastError());
    if (int rc = reads_layout_windows(d_klen, n_kept, keep_quality, st, F)) return rc;
    if (int rc = write_windows(reads, d_ksrc, nullptr, F, st)) return rc;
    if (O.kept) HIP_TRY(hipMemcpyAsync(O.kept, d_ksrc, n_kept * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the handle is whole when the call returns, and the area is free again)
    n_groups = (size_t)n_kept;
    launches += 10u;  // the score and the keep kernel, the scan's three, the compaction, the layout scan's three, the write kernel
  }
  s->stats.scan_launches = launches;
  if (O.n_unique) *O.n_unique = n_unique;
  if (O.n_groups) *O.n_groups = n_groups;
  return 0;
}

int dedup_call(sassy_SearcherType* s, const sassy_hip_Reads* reads, uint32_t at, size_t m, size_t k, uint32_t method, uint32_t flags, const DdpOut& O,
               bool have_out, sassy_hip_Reads** out_dedup, const char* who) {
  DdpCall c{};
  c.have_searcher = s != nullptr; c.have_out = have_out;
  c.flags = flags; c.method = method; c.at = at; c.m = m;
  c.gate = reads_gate_of(s, 1, reads, nullptr);
  // the searcher and the numbers first: the batch is read only once nothing in front of it is wrong
  ReadsRefusal gate = kRdsOk;
  DdpRefusal why = ddp_refusal(c, &gate);
  if (why == kDdpOk || why == kDdpNullOut || (why == kDdpGate && gate == kRdsInFlight)) {
    reads_gate_read(s, reads, nullptr, &c.gate);
    why = ddp_refusal(c, &gate);
  }
  if (why == kDdpGate)
    return reads_refused(gate, c.gate, ReadsWho{who, "the keys are DNA", "compares windows that lie inside the reads", "groups every read"});
  if (why != kDdpOk) return fail(SASSY_HIP_EINVAL, refusal_text(why, c, who));
  return reads_new_batch(s, m, k, out_dedup, [&](uint32_t kk, sassy_hip_Reads* F) {  // (k >= m: every two distinct keys are neighbours)
    return pairs_guarded(who, [&]() -> int { return dedup_run(s, reads, at, (uint32_t)m, kk, method, flags, O, F, who); });
  });
}

}  // namespace
}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_umi_groups_reads(sassy_SearcherType* s, const sassy_hip_Reads* reads, uint32_t at, size_t m, size_t k, uint32_t method, uint32_t flags,
                               uint32_t* out_label, uint32_t* out_size, uint32_t* out_rep, uint32_t* out_count, size_t* n_unique, size_t* n_groups) {
  const DdpOut O{out_label, out_size, out_rep, out_count, nullptr, n_unique, n_groups};
  return dedup_call(s, reads, at, m, k, method, flags, O, out_label != nullptr, nullptr, "umi_groups_reads");
}

int sassy_hip_dedup_reads(sassy_SearcherType* s, const sassy_hip_Reads* reads, uint32_t at, size_t m, size_t k, uint32_t method, uint32_t flags,
                          uint32_t* out_label, uint32_t* out_size, uint32_t* out_rep, uint32_t* out_count, uint64_t* out_kept, size_t* n_unique,
                          size_t* n_groups, sassy_hip_Reads** out_dedup) {
  if (out_dedup) *out_dedup = nullptr;
  const DdpOut O{out_label, out_size, out_rep, out_count, out_kept, n_unique, n_groups};
  return dedup_call(s, reads, at, m, k, method, flags, O, out_dedup != nullptr, out_dedup, "dedup_reads");
}

}  // extern "C"
