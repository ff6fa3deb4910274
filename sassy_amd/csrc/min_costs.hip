// min_costs.hip -- best-cost search: sassy_hip_min_costs / sassy_hip_best_pattern.  Where search_many runs a batch of host
// texts in one pass (many_patterns.hip: search_many_batched, search_many_pertext) the scan's (pattern, position, cost) list
// is reduced here to one 32-bit cell per (pattern, text) pair or per text -- no sort, no report rule, no traceback, no
// records; everything else runs search_many and its records are reduced on the host.  DESIGN.md 5.6b.
#include "host_internal.h"

namespace sassy_hip {

constexpr uint32_t kNoCell = 0xFFFFFFFFu;  // a cell nothing matched; the cell index of a lane without an entry

struct MinReduceParams {
  const Candidate* list;
  uint32_t count;
  TextTable T;        // the strand's text table (the Rc strand's list refers to the reversed buffer)
  uint32_t* cells;
  uint64_t n_cells;
  uint64_t n_cols;    // texts of the whole call: the row length of the pair matrix
  uint64_t col0;      // the batch's first text
  uint32_t nt;        // texts in the batch
  uint32_t flip;      // the list is of the batch reversed as a whole (the Rc strand's pass): its text r is text nt - 1 - r
  uint32_t strand;
  uint32_t per_text;  // 1: one cell per text, key = cost << 25 | pattern << 1 | strand; 0: per pair, key = cost << 1 | strand
};

// One lane per list entry.  entry -> text (the largest t with start[t] <= position, as assign_texts_kernel: an entry in the
// separator or the virtual columns behind a text belongs to that text -- costs never fall across a separator, so it cannot
// undercut the text's own entries) -> cell and packed key: ONE unsigned min implements the whole tie rule (lowest cost,
// then lowest pattern, then Fwd).  The entries of a wave are neighbours in the text (the tiled scan lists runs of positions
// of one pattern, the seeded search the hits of one stretch), so runs of lanes share a cell: a segmented min-scan over
// the lanes leaves each run's minimum in its last lane, which looks at the cell and sends an atomic only if it would
// lower it (cells only ever fall: a stale look costs an atomic, never a result).
__global__ __launch_bounds__(256) void min_reduce_kernel(const MinReduceParams P) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t cell = kNoCell, key = kNoCell;
  if (i < P.count) {
    const Candidate v = P.list[i];
    uint32_t lo = 0, hi = P.T.n;  // invariant: start[lo] <= pos < start[hi]
    while (lo + 1 < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (P.T.start[mid] <= v.pos) lo = mid; else hi = mid;
    }
    const uint64_t col = P.col0 + (P.flip ? P.nt - 1u - lo : lo);
    const uint32_t pat = v.flags >> kCandTextShift;
    const uint64_t c = P.per_text ? col : (uint64_t)pat * P.n_cols + col;
    if (c < P.n_cells && col < P.n_cols) {
      cell = (uint32_t)c;
      key = P.per_text ? ((uint32_t)v.cost << 25) | (pat << 1) | P.strand : ((uint32_t)v.cost << 1) | P.strand;
    }
  }
  const uint32_t before = __shfl_up(cell, 1);
  uint32_t joined = (lane == 0 || before != cell) ? 1u : 0u;  // 1: the scan has reached the first lane of this lane's run
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t key_up = __shfl_up(key, d), joined_up = __shfl_up(joined, d);
    if (lane >= d && !joined) {
      key = min(key, key_up);
      joined = joined_up;
    }
  }
  const uint32_t behind = __shfl_down(cell, 1);
  if ((lane == 63 || behind != cell) && cell != kNoCell)
    if (P.cells[cell] > key) atomicMin(P.cells + cell, key);
}

// cells -> the outputs' types.  Per pair: four cells per thread, cost bytes at out, strand bytes at out + plane.
__global__ __launch_bounds__(256) void min_narrow_pairs_kernel(const uint4* __restrict__ cells, uint64_t n4, uint32_t* __restrict__ out_cost,
                                                               uint32_t* __restrict__ out_strand) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const uint4 c = cells[i];
  const uint32_t v[4] = {c.x, c.y, c.z, c.w};
  uint32_t cost = 0, strand = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cost |= (v[j] == kNoCell ? SASSY_HIP_NO_MATCH : (v[j] >> 1) & 0xFFu) << (8 * j);
    strand |= (v[j] == kNoCell ? 0u : v[j] & 1u) << (8 * j);
  }
  out_cost[i] = cost;
  out_strand[i] = strand;
}
// Per text: pattern words at out_pattern, cost and strand bytes behind them.
__global__ __launch_bounds__(256) void min_narrow_texts_kernel(const uint32_t* __restrict__ cells, uint64_t n, uint32_t* __restrict__ out_pattern,
                                                               uint8_t* __restrict__ out_cost, uint8_t* __restrict__ out_strand) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cells[i];
  out_pattern[i] = c == kNoCell ? 0xFFFFFFFFu : (c >> 1) & 0xFFFFFFu;
  out_cost[i] = (uint8_t)(c == kNoCell ? SASSY_HIP_NO_MATCH : c >> 25);
  out_strand[i] = (uint8_t)(c == kNoCell ? 0u : c & 1u);
}

// The list of one strand's pass over a batch (s->d_tiled_list, `count` entries) into the cells of the call in progress.
int reduce_pattern_list(sassy_SearcherType* s, uint32_t count, const TextTable* tt) {
  MinSink* sink = s->min_sink;
  if (!sink || !sink->armed || (!sink->d_cells && !sink->d_located) || !tt || tt->n == 0)
    return fail(SASSY_HIP_EINVAL, "internal: list reduction without a batch of texts");
  MinReduceParams P{};
  P.list = s->d_tiled_list.p;
  P.count = count;
  P.T = *tt;
  P.cells = sink->d_cells;
  P.n_cols = sink->n_cols;
  P.n_cells = sink->n_cells;
  P.col0 = sink->col0;
  P.nt = sink->nt;
  P.flip = (sink->flip && sink->strand) ? 1u : 0u;  // (only the Rc strand's pass reads the reversed buffer)
  P.strand = sink->strand;
  P.per_text = sink->per_text ? 1u : 0u;
  hipStream_t st = s->stream;
  const bool timed = s->timing >= 2;
  if (timed) HIP_TRY(hipEventRecord(s->ev_a_multi(), st));
  hipError_t le;
  if (sink->d_located) {  // (best_matches: the cell keeps the end position too -- best_matches.hip)
    MinSink one = *sink;
    one.flip = P.flip != 0;
    le = launch_locate_reduce(P.list, count, *tt, one, st);
  } else {
    hipLaunchKernelGGL(min_reduce_kernel, dim3((uint32_t)(((uint64_t)count + 255) / 256)), dim3(256), 0, st, P);  // (lists hold at most 2^28 + 2^27 entries)
    le = hipGetLastError();
  }
  if (le != hipSuccess) return hip_fail(le, "list reduction launch");
  if (timed) {
    HIP_TRY(hipEventRecord(s->ev_multi, st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev_a_multi(), s->ev_multi));
    s->stats.trace_ms += ms;
  }
  sink->used = true;
  return 0;
}

namespace {

// out_pattern == nullptr: the pair matrix (sassy_hip_min_costs); else one row per text (sassy_hip_best_pattern; the caller
// passes buffers of its own for the outputs its caller left out).
int best_costs(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns, TextSource& src,
               size_t k, uint32_t flags, bool per_text, uint8_t* out_cost, uint32_t* out_pattern, uint8_t* out_strand) {
  const size_t n_texts = src.n;
  if (!s || !out_cost || (n_patterns && (!patterns || !pattern_lens)) || (n_texts && (!src.texts || !src.lens)))
    return fail(SASSY_HIP_EINVAL, "null argument");
  SASSY_NO_LINE_SPANS(flags);
  if (flags & ~SASSY_HIP_TEXT_ON_DEVICE) return fail(SASSY_HIP_EINVAL, "best-cost search takes SASSY_HIP_TEXT_ON_DEVICE only");
  if (k > 254) return fail(SASSY_HIP_EINVAL, "best-cost search: k must be <= 254 (costs are bytes, 255 = no match)");
  SASSY_NO_TICKETS(s);
  const double t0 = now_ms();
  const size_t n_out = per_text ? n_texts : n_patterns * n_texts;
  // ---- the device path: a batch of host texts or a resident read batch, patterns of one length (what the one-pass paths of
  // search_many take) ----
  bool device = s->sw.min_cost_device != 0 && n_texts >= 2 && n_patterns > 0 && (!(flags & SASSY_HIP_TEXT_ON_DEVICE) || src.reads) &&
                !is_ascii(s->profile) && pattern_lens[0] <= 64 && 2 * k + 3 <= 64 &&
                (per_text ? n_patterns < (1u << 24) : (uint64_t)n_patterns * n_texts <= 0xFFFFFF00ull);
  for (size_t pi = 1; device && pi < n_patterns; ++pi) device = pattern_lens[pi] == pattern_lens[0];
  MinSink sink;
  const size_t n_cells = (n_out + 15) / 16 * 16;
  if (device) {
    DeviceGuard on_device(s);
    if (int rc = s->ensure_device()) return rc;
    if (s->d_min_cells.reserve(n_cells) != 0) {
      (void)hipGetLastError();
      return fail(SASSY_HIP_ENOMEM, "best-cost search: no device memory for " + std::to_string(n_cells * 4) + " bytes of cost cells");
    }
    HIP_TRY(hipMemsetAsync(s->d_min_cells.p, 0xFF, n_cells * 4, s->stream));
    sink.d_cells = s->d_min_cells.p;
    sink.per_text = per_text;
    sink.n_cols = n_texts;
    sink.n_cells = n_out;
    s->min_sink = &sink;
  }
  // (the traced span decides the N filter: only without it can the traceback be left out)
  const uint32_t many_flags = flags | (std::isnan(s->max_n_frac) ? SASSY_HIP_WITHOUT_TRACE : 0u);
  sassy_hip_Result* R = nullptr;
  const int rc_many = search_many_source(s, patterns, pattern_lens, n_patterns, src, k, many_flags, &R);
  s->min_sink = nullptr;
  if (rc_many) return rc_many;
  std::unique_ptr<sassy_hip_Result> owned(R);
  memset(out_cost, (int)SASSY_HIP_NO_MATCH, n_out);
  if (out_strand) memset(out_strand, 0, n_out);
  if (per_text)
    for (size_t t = 0; t < n_texts; ++t) out_pattern[t] = 0xFFFFFFFFu;
  // ---- what the device reduced ----
  if (sink.used) {
    DeviceGuard on_device(s);
    hipStream_t st = s->stream;
    const bool timed = s->timing >= 2;
    if (timed) HIP_TRY(hipEventRecord(s->ev_a_multi(), st));
    if (per_text) {
      if (int rc = s->d_min_out.reserve(6 * n_cells)) return rc;
      uint32_t* d_pat = reinterpret_cast<uint32_t*>(s->d_min_out.p);
      uint8_t* d_cost = s->d_min_out.p + 4 * n_cells;
      uint8_t* d_strand = d_cost + n_cells;
      hipLaunchKernelGGL(min_narrow_texts_kernel, dim3((uint32_t)((n_out + 255) / 256)), dim3(256), 0, st, s->d_min_cells.p, (uint64_t)n_out,
                         d_pat, d_cost, d_strand);
      hipError_t le = hipGetLastError();
      if (le != hipSuccess) return hip_fail(le, "cost narrowing launch");
      if (timed) HIP_TRY(hipEventRecord(s->ev_multi, st));
      HIP_TRY(hipMemcpyAsync(out_cost, d_cost, n_out, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(out_pattern, d_pat, n_out * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(out_strand, d_strand, n_out, hipMemcpyDeviceToHost, st));
    } else {
      if (int rc = s->d_min_out.reserve(2 * n_cells)) return rc;
      uint8_t* d_cost = s->d_min_out.p;
      uint8_t* d_strand = d_cost + n_cells;
      const uint64_t n4 = n_cells / 4;
      hipLaunchKernelGGL(min_narrow_pairs_kernel, dim3((uint32_t)((n4 + 255) / 256)), dim3(256), 0, st,
                         reinterpret_cast<const uint4*>(s->d_min_cells.p), n4, reinterpret_cast<uint32_t*>(d_cost),
                         reinterpret_cast<uint32_t*>(d_strand));
      hipError_t le = hipGetLastError();
      if (le != hipSuccess) return hip_fail(le, "cost narrowing launch");
      if (timed) HIP_TRY(hipEventRecord(s->ev_multi, st));
      HIP_TRY(hipMemcpyAsync(out_cost, d_cost, n_out, hipMemcpyDeviceToHost, st));
      if (out_strand) HIP_TRY(hipMemcpyAsync(out_strand, d_strand, n_out, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (timed) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, s->ev_a_multi(), s->ev_multi));
      s->stats.trace_ms += ms;
    }
  }
  // ---- what came back as records (the general path; a batch the one-pass paths declined or could not finish) ----
  const sassy_hip_Match* rows = owned->data();
  for (size_t i = 0, n = owned->size(); i < n; ++i) {
    const sassy_hip_Match& r = rows[i];
    if (r.pattern_idx >= n_patterns || r.text_idx >= n_texts || r.cost < 0 || r.cost > 254) continue;
    const uint8_t cost = (uint8_t)r.cost, strand = r.strand ? 1 : 0;
    if (per_text) {
      const size_t t = (size_t)r.text_idx;
      const uint32_t pat = (uint32_t)r.pattern_idx;
      const bool better = cost < out_cost[t] || (cost == out_cost[t] && (pat < out_pattern[t] || (pat == out_pattern[t] && strand < out_strand[t])));
      if (better) {
        out_cost[t] = cost;
        out_pattern[t] = pat;
        out_strand[t] = strand;
      }
    } else {
      const size_t c = (size_t)r.pattern_idx * n_texts + (size_t)r.text_idx;
      if (cost < out_cost[c] || (cost == out_cost[c] && out_strand && strand < out_strand[c])) {
        out_cost[c] = cost;
        if (out_strand) out_strand[c] = strand;
      }
    }
  }
  s->stats.total_ms = now_ms() - t0;
  s->stats.host_post_ms = s->stats.total_ms - s->stats.host_enqueue_ms - s->stats.host_wait_ms;
  return 0;
}

}  // namespace
}  // namespace sassy_hip

extern "C" {

// (nothing may leave through the C ABI: a failed allocation of the host's scratch is SASSY_HIP_ENOMEM)
int sassy_hip_min_costs(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                        const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags,
                        uint8_t* out_cost, uint8_t* out_strand) {
  try {
    TextSource src{texts, text_lens, n_texts};
    return best_costs(s, patterns, pattern_lens, n_patterns, src, k, flags, false, out_cost, nullptr, out_strand);
  } catch (const std::bad_alloc&) {
    if (s) s->min_sink = nullptr;
    return fail(SASSY_HIP_ENOMEM, "best-cost search: out of host memory");
  }
}

int sassy_hip_min_costs_reads(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                              const sassy_hip_Reads* reads, size_t k, uint32_t flags, uint8_t* out_cost, uint8_t* out_strand) {
  try {
    ReadsTexts rt;
    if (int rc = reads_as_source(s, reads, flags, "min_costs_reads", &rt)) return rc;
    return best_costs(s, patterns, pattern_lens, n_patterns, rt.src, k, flags | SASSY_HIP_TEXT_ON_DEVICE, false, out_cost, nullptr, out_strand);
  } catch (const std::bad_alloc&) {
    if (s) s->min_sink = nullptr;
    return fail(SASSY_HIP_ENOMEM, "best-cost search: out of host memory");
  }
}

int sassy_hip_best_pattern(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                           const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags,
                           uint8_t* out_cost, uint32_t* out_pattern, uint8_t* out_strand) {
  try {
    // (the tie rule needs pattern and strand of the best so far, whether the caller wants them or not)
    std::vector<uint32_t> pat_tmp;
    std::vector<uint8_t> strand_tmp;
    if (!out_pattern) { pat_tmp.resize(n_texts + 1); out_pattern = pat_tmp.data(); }
    if (!out_strand) { strand_tmp.resize(n_texts + 1); out_strand = strand_tmp.data(); }
    TextSource src{texts, text_lens, n_texts};
    return best_costs(s, patterns, pattern_lens, n_patterns, src, k, flags, true, out_cost, out_pattern, out_strand);
  } catch (const std::bad_alloc&) {
    if (s) s->min_sink = nullptr;
    return fail(SASSY_HIP_ENOMEM, "best-cost search: out of host memory");
  }
}

int sassy_hip_best_pattern_reads(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                 const sassy_hip_Reads* reads, size_t k, uint32_t flags, uint8_t* out_cost, uint32_t* out_pattern,
                                 uint8_t* out_strand) {
  try {
    ReadsTexts rt;
    if (int rc = reads_as_source(s, reads, flags, "best_pattern_reads", &rt)) return rc;
    const size_t n_texts = rt.src.n;
    std::vector<uint32_t> pat_tmp;
    std::vector<uint8_t> strand_tmp;
    if (!out_pattern) { pat_tmp.resize(n_texts + 1); out_pattern = pat_tmp.data(); }
    if (!out_strand) { strand_tmp.resize(n_texts + 1); out_strand = strand_tmp.data(); }
    return best_costs(s, patterns, pattern_lens, n_patterns, rt.src, k, flags | SASSY_HIP_TEXT_ON_DEVICE, true, out_cost, out_pattern, out_strand);
  } catch (const std::bad_alloc&) {
    if (s) s->min_sink = nullptr;
    return fail(SASSY_HIP_ENOMEM, "best-cost search: out of host memory");
  }
}

}  // extern "C"
