// best_matches.hip -- sassy_hip_best_matches: per text the one best match, located and traced.  Where search_many runs a
// batch of host texts in one pass (many_patterns.hip: search_many_batched, search_many_pertext) the scan's (pattern,
// position, cost) list is reduced here to one 64-bit cell per text that keeps the winning end position, every non-empty
// cell becomes one traceback candidate, and the existing tail traces and assembles one record per text
// (many_patterns.hip: finish_best_matches).  Everything else runs search_many and its records are reduced on the host by
// the same order.  DESIGN.md 5.6c.
#include "host_internal.h"

namespace sassy_hip {

// The key of an entry, smaller = better:
//   bits 56..63 cost | 32..55 pattern | 31 strand | 0..30 0x7FFFFFFF - end
// end = the entry's end position within its text in scan coordinates (the Rc strand's list refers to the reversed text), so
// ONE unsigned 64-bit min implements lowest cost, lowest pattern, Fwd before Rc, rightmost end.  A cell nothing matched
// holds all ones (cost <= 254: no key does).
struct LocateParams {
  const Candidate* list;
  uint32_t count;
  TextTable T;        // the strand's text table
  unsigned long long* cells;
  uint64_t n_cells;   // texts of the whole call
  uint64_t col0;      // the batch's first text
  uint32_t nt;        // texts in the batch
  uint32_t flip;      // the list is of the batch reversed as a whole: its text r is text nt - 1 - r
  uint32_t strand;
};

constexpr uint32_t kNoText = 0xFFFFFFFFu;  // the cell index of a lane without an entry

// min_reduce_kernel's shape (min_costs.hip) with a 64-bit key: a lane per list entry; entry -> text by binary search in
// the strand's table (an entry in the separator or the padding behind a text belongs to that text and counts as its end --
// costs never fall across a separator, so the text's end has the same cost when such an entry is a minimum: what
// assign_texts_kernel does to a report; overhang: the virtual columns up to len + ov_steps are end positions of their own
// and keep their place); a segmented min-scan over the runs of lanes that share a cell; the run's last lane looks at the
// cell and sends the atomic only if it would lower it.
__global__ __launch_bounds__(256) void locate_reduce_kernel(const LocateParams P) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t cell = kNoText;
  unsigned long long key = kNoLocated;
  if (i < P.count) {
    const Candidate v = P.list[i];
    uint32_t lo = 0, hi = P.T.n;  // invariant: start[lo] <= pos < start[hi]
    while (lo + 1 < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (P.T.start[mid] <= v.pos) lo = mid; else hi = mid;
    }
    const uint64_t col = P.col0 + (P.flip ? P.nt - 1u - lo : lo);
    const uint64_t start = P.T.start[lo], len = P.T.len[lo];
    uint64_t end = v.pos >= start ? v.pos - start : 0;
    if (end > len + P.T.ov_steps) end = len;
    const uint32_t pat = v.flags >> kCandTextShift;
    if (col < P.n_cells && col < kNoText && end <= 0x7FFFFFFFull && (uint32_t)v.cost < 255u) {
      cell = (uint32_t)col;
      key = ((unsigned long long)(uint32_t)v.cost << 56) | ((unsigned long long)pat << 32) | ((unsigned long long)P.strand << 31) |
            (0x7FFFFFFFull - end);
    }
  }
  const uint32_t before = __shfl_up(cell, 1);
  uint32_t joined = (lane == 0 || before != cell) ? 1u : 0u;  // 1: the scan has reached the first lane of this lane's run
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t hi_up = __shfl_up((uint32_t)(key >> 32), d), lo_up = __shfl_up((uint32_t)key, d), joined_up = __shfl_up(joined, d);
    const unsigned long long key_up = ((unsigned long long)hi_up << 32) | lo_up;
    if (lane >= d && !joined) {
      key = key_up < key ? key_up : key;
      joined = joined_up;
    }
  }
  const uint32_t behind = __shfl_down(cell, 1);
  if ((lane == 63 || behind != cell) && cell != kNoText)
    if (P.cells[cell] > key) atomicMin(P.cells + cell, key);
}

// cells -> candidates: a lane per text of the batch.  A non-empty cell gives {absolute end position in its strand's buffer,
// cost, pattern << kCandTextShift} and the text's index in that strand's table; the waves append to the two strands' lists
// with one atomic per wave and strand (the order does not matter: the assembly sorts by text).
struct BestCandParams {
  const unsigned long long* cells;  // the batch's first cell
  uint32_t nt;
  TextTable T[2];
  uint32_t flip;
  Candidate* cand;   // strand s: cand + s * nt
  uint32_t* rtext;   // strand s: rtext + s * nt
  uint32_t* count;   // [2]
};
__global__ __launch_bounds__(256) void best_candidates_kernel(const BestCandParams P) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long c = kNoLocated;
  if (t < P.nt) c = P.cells[t];
  const bool have = c != kNoLocated;
  const uint32_t strand = (uint32_t)(c >> 31) & 1u;
#pragma unroll
  for (uint32_t sd = 0; sd < 2; ++sd) {
    const bool mine = have && strand == sd;
    const unsigned long long mask = __ballot(mine);
    if (mask == 0) continue;  // (wave-uniform)
    const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(P.count + sd, (uint32_t)__popcll(mask));
    base = __shfl(base, (int)leader);
    if (mine) {
      const uint32_t slot = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      const uint32_t r = (sd && P.flip) ? P.nt - 1u - t : t;
      if (slot < P.nt) {
        Candidate v;
        v.pos = P.T[sd].start[r] + (0x7FFFFFFFull - (c & 0x7FFFFFFFull));
        v.cost = (int32_t)(c >> 56);
        v.flags = ((uint32_t)(c >> 32) & 0xFFFFFFu) << kCandTextShift;
        P.cand[(size_t)sd * P.nt + slot] = v;
        P.rtext[(size_t)sd * P.nt + slot] = r;
      }
    }
  }
}

hipError_t launch_locate_reduce(const Candidate* d_list, uint32_t count, const TextTable& texts, const MinSink& sink, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  LocateParams P{};
  P.list = d_list;
  P.count = count;
  P.T = texts;
  P.cells = sink.d_located;
  P.n_cells = sink.n_cells;
  P.col0 = sink.col0;
  P.nt = sink.nt;
  P.flip = sink.flip ? 1u : 0u;
  P.strand = sink.strand;
  hipLaunchKernelGGL(locate_reduce_kernel, dim3((uint32_t)(((uint64_t)count + 255) / 256)), dim3(256), 0, stream, P);
  return hipGetLastError();
}

hipError_t launch_best_candidates(const unsigned long long* d_cells, uint32_t nt, const TextTable& fwd, const TextTable& rcs, uint32_t flip,
                                  Candidate* d_cand, uint32_t* d_rtext, uint32_t* d_count, hipStream_t stream) {
  if (nt == 0) return hipSuccess;
  BestCandParams P{};
  P.cells = d_cells;
  P.nt = nt;
  P.T[0] = fwd;
  P.T[1] = rcs;
  P.flip = flip;
  P.cand = d_cand;
  P.rtext = d_rtext;
  P.count = d_count;
  hipLaunchKernelGGL(best_candidates_kernel, dim3((nt + 255) / 256), dim3(256), 0, stream, P);
  return hipGetLastError();
}

namespace {

// Is record a better than record b of the same text?  The definition's order: lowest cost, lowest pattern, Fwd before Rc,
// the rightmost end in the strand's scan direction -- the largest text_end for Fwd, the smallest text_start for Rc (the Rc
// strand is scanned on the reversed text); of two overhang matches that end behind the text's end, the one that hangs
// over further (the smaller pattern_end) ends further right.  Without trace the records carry exactly these fields.
bool better_match(const sassy_hip_Match& a, const sassy_hip_Match& b) {
  if (a.cost != b.cost) return a.cost < b.cost;
  if (a.pattern_idx != b.pattern_idx) return a.pattern_idx < b.pattern_idx;
  if (a.strand != b.strand) return a.strand < b.strand;
  if (a.strand) {
    if (a.text_start != b.text_start) return a.text_start < b.text_start;
  } else {
    if (a.text_end != b.text_end) return a.text_end > b.text_end;
  }
  return a.pattern_end < b.pattern_end;
}

int best_matches(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns, TextSource& src,
                 size_t k, uint32_t flags, sassy_hip_Result** out) {
  const size_t* text_lens = src.lens;
  const size_t n_texts = src.n;
  if (!s || !out || (n_patterns && (!patterns || !pattern_lens)) || (n_texts && (!src.texts || !text_lens)))
    return fail(SASSY_HIP_EINVAL, "null argument");
  SASSY_NO_LINE_SPANS(flags);
  if (flags & ~(SASSY_HIP_TEXT_ON_DEVICE | SASSY_HIP_WITHOUT_TRACE))
    return fail(SASSY_HIP_EINVAL, "best_matches takes SASSY_HIP_TEXT_ON_DEVICE and SASSY_HIP_WITHOUT_TRACE only");
  if (k > 254) return fail(SASSY_HIP_EINVAL, "best_matches: k must be <= 254 (as best_pattern: costs are bytes, 255 = no match)");
  SASSY_NO_TICKETS(s);
  if (s->rc && is_ascii(s->profile) && n_patterns && n_texts)
    return fail(SASSY_HIP_EUNSUPPORTED, "reverse complement is not defined for the ascii alphabet");
  const double t0 = now_ms();
  // ---- the device path: where best_pattern's device reduction takes the call, without the N filter, texts < 2^31 ----
  bool device = s->sw.best_match_device != 0 && n_texts >= 2 && n_patterns > 0 && (!(flags & SASSY_HIP_TEXT_ON_DEVICE) || src.reads) &&
                !is_ascii(s->profile) && pattern_lens[0] <= 64 && 2 * k + 3 <= 64 && n_patterns < (1u << 24) &&
                std::isnan(s->max_n_frac);
  for (size_t pi = 1; device && pi < n_patterns; ++pi) device = pattern_lens[pi] == pattern_lens[0];
  for (size_t ti = 0; device && ti < n_texts; ++ti) device = text_lens[ti] < (1ull << 31) - 128;  // (the end position: 31 bits, virtual columns included)
  MinSink sink;
  if (device) {
    DeviceGuard on_device(s);
    if (int rc = s->ensure_device()) return rc;
    if (s->d_best_cells.reserve(n_texts) != 0) {
      (void)hipGetLastError();
      return fail(SASSY_HIP_ENOMEM, "best_matches: no device memory for " + std::to_string(n_texts * 8) + " bytes of cells");
    }
    HIP_TRY(hipMemsetAsync(s->d_best_cells.p, 0xFF, n_texts * 8, s->stream));
    sink.d_located = s->d_best_cells.p;
    sink.per_text = true;
    sink.n_cols = n_texts;
    sink.n_cells = n_texts;
    sink.without_trace = (flags & SASSY_HIP_WITHOUT_TRACE) != 0;
    s->min_sink = &sink;
  }
  // (the definition reduces the records of a searcher with only_best_match off)
  struct Restore {
    sassy_SearcherType* s; bool only_best;
    ~Restore() { s->only_best = only_best; s->min_sink = nullptr; }
  } restore{s, s->only_best};
  s->only_best = false;
  sassy_hip_Result* R = nullptr;
  if (int rc = search_many_source(s, patterns, pattern_lens, n_patterns, src, k, flags, &R)) return rc;
  std::unique_ptr<sassy_hip_Result> all(R);
  if (sink.located) {  // (records the host made -- without trace -- went through search_many's pattern-major sort)
    std::sort(all->matches.begin(), all->matches.end(),
              [](const sassy_hip_Match& a, const sassy_hip_Match& b) { return a.text_idx < b.text_idx; });
  } else {
    // ---- the general path: search_many's records reduced by the definition ----
    const sassy_hip_Match* rows = all->data();
    std::vector<size_t> best(n_texts, SIZE_MAX);
    for (size_t i = 0, n = all->size(); i < n; ++i) {
      const sassy_hip_Match& r = rows[i];
      if (r.text_idx >= n_texts) continue;
      size_t& b = best[(size_t)r.text_idx];
      if (b == SIZE_MAX || better_match(r, rows[b])) b = i;
    }
    std::unique_ptr<sassy_hip_Result> B(new sassy_hip_Result());
    const char* pool = all->pool_data();
    for (size_t t = 0; t < n_texts; ++t) {
      if (best[t] == SIZE_MAX) continue;
      sassy_hip_Match r = rows[best[t]];
      const size_t off = B->pool.size();
      if (off + r.cigar_len + 1 > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "cigar pool of one result exceeds 4 GiB");
      B->pool.append(pool + r.cigar_off, r.cigar_len);
      B->pool.push_back('\0');
      r.cigar_off = (uint32_t)off;
      B->matches.push_back(r);
    }
    if (B->pool.empty()) B->pool.push_back('\0');
    all = std::move(B);
  }
  s->stats.total_ms = now_ms() - t0;
  s->stats.host_post_ms = s->stats.total_ms - s->stats.host_enqueue_ms - s->stats.host_wait_ms;
  *out = all.release();
  return 0;
}

}  // namespace
}  // namespace sassy_hip

extern "C" {

// (nothing may leave through the C ABI: a failed allocation of the host's scratch is SASSY_HIP_ENOMEM)
int sassy_hip_best_matches(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                           const uint8_t* const* texts, const size_t* text_lens, size_t n_texts, size_t k, uint32_t flags,
                           sassy_hip_Result** out) {
  try {
    TextSource src{texts, text_lens, n_texts};
    return best_matches(s, patterns, pattern_lens, n_patterns, src, k, flags, out);
  } catch (const std::bad_alloc&) {
    if (s) s->min_sink = nullptr;
    return fail(SASSY_HIP_ENOMEM, "best_matches: out of host memory");
  }
}

int sassy_hip_best_matches_reads(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns,
                                 const sassy_hip_Reads* reads, size_t k, uint32_t flags, sassy_hip_Result** out) {
  try {
    if (out) *out = nullptr;
    ReadsTexts rt;
    if (int rc = reads_as_source(s, reads, flags, "best_matches_reads", &rt)) return rc;
    return best_matches(s, patterns, pattern_lens, n_patterns, rt.src, k, flags | SASSY_HIP_TEXT_ON_DEVICE, out);
  } catch (const std::bad_alloc&) {
    if (s) s->min_sink = nullptr;
    return fail(SASSY_HIP_ENOMEM, "best_matches: out of host memory");
  }
}

}  // extern "C"
