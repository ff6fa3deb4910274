// trim_reads.hip -- the 3' adapter and the low-quality tail cut off every read of a resident read batch, what is left too
// short dropped, into a NEW resident read batch (sassy_hip_trim_reads), and a host-given window of every read
// as a new batch (sassy_hip_reads_slice).  Record r of the result is what is left of read r, empty where it was dropped, so
// an index means the same read in both handles.  The arithmetic -- the refusals, the quality walk, the planes, the
// mismatches of a position, the order, the record, a block of a window -- is trim_step.h's; the acceptance rule is
// overlap_step.h's (ovl_accepts); the layout rule and its scan are the parse's (fastq_reads.hip: reads_layout_trimmed,
// reads_layout_windows).
//
// Device work of a trim, all on the searcher's stream:
//   trim_find_kernel     one wavefront per read, four reads per workgroup.
//     quality  (asked for only) 64 bytes a round from the read's far end, a lane per byte: the signed terms, a suffix scan
//              over the wavefront with the sum of the rounds behind it, the highest lane with s > 0 by ballot, and per lane
//              the lowest s above it; a butterfly leaves lq.
//     planes   64 bytes per step, a lane per byte: the lane's code, one ballot per plane and one for VALID (rows below lq);
//              the words go to LDS with two zero words behind every plane.
//     positions the lanes become positions c, 64 a round: per plane three LDS words and two funnel shifts by c mod 32, once
//              per round; per adapter (its table entry is wave-uniform: scalar loads) the mismatch words under
//              VALID & the adapter's valid rows, two popcounts, ovl_accepts, trm_combine.  A round that accepts a position
//              ends the walk: no later round holds a smaller c.
//     result   a butterfly over the wavefront with trm_combine; lane 0 stores the 16-byte record.
//   fastq_rec_sum / _top / _write_kernel    the lengths from the records, starts = the exclusive scan of them rounded up to 64,
//                                           the record table, the longest read, the layout's size  -> host (one wait)
//   reads_window_write_kernel   a lane per 64-byte block of the OUTPUT, as fastq_copy_kernel and merge_write_kernel: the block's
//              read by ham_text_of over the new starts, its 64 bytes from [begin, begin + length) of the source read -- a slice
//              (SHIFTED): five 16-byte loads shifted by fq_shift_block; a trim (not SHIFTED: begin = 0, so source and block are
//              64-byte aligned): four aligned loads per buffer, all issued before the first store; every load bounded by the source's text size --,
//              four 16-byte stores into the text and, where kept, the quality buffer, zeros behind the read's end, rem[block];
//              one extra lane zeroes the 64 spare bytes.  No buffer is cleared as a whole.
//              GATHER (demux_reads.hip: a select, a demux): the block's read comes from read src[t] of the source handle.
// The input handle is only read.  Every load of a read's bytes is bounded by the handle's length table and its text size,
// every store by the block count.
#include <hip/hip_runtime.h>

#include "host_internal.h"
#include "fastq_step.h"
#include "hamming_step.h"
#include "trim_step.h"

static_assert(sizeof(sassy_hip_ReadTrim) == 16 && sizeof(sassy_hip::TrmRecord) == 16, "one 16-byte store per read");
static_assert(offsetof(sassy_hip_ReadTrim, adapter) == 12 && offsetof(sassy_hip_ReadTrim, overlap) == 14 && offsetof(sassy_hip_ReadTrim, mismatches) == 15,
              "TrmRecord::tail is the record's last word");
static_assert(SASSY_HIP_TRIM_MAX_ADAPTERS == sassy_hip::kTrmMaxAdapters, "the header's limit is the step header's");

namespace sassy_hip {
namespace {

struct TrimArgs {
  const uint8_t *text, *qual;
  const uint64_t *start, *len;  // the handle's tables
  uint64_t bytes;               // the handle's text size
  uint64_t n;
  const uint32_t* tab;          // n_adapters entries of kTrmTableWords words
  uint32_t n_adapters, min_overlap, k, max_permille, cutoff, min_length;
  TrmRecord* out;
};

template <int W, bool IUPAC>
__global__ __launch_bounds__(256) void trim_find_kernel(TrimArgs A) {
  constexpr int P = IUPAC ? 4 : 2;
  constexpr uint32_t profile = IUPAC ? kHamIupac : kHamDna;
  constexpr uint32_t S = W + kTrmPad;  // words of a plane in LDS
  __shared__ uint32_t lds[kTrmReadsPerGroup][(P + 1) * S];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t read = (uint64_t)blockIdx.x * kTrmReadsPerGroup + wave;
  const bool live = read < A.n;
  uint32_t* planes = lds[wave];

  uint64_t s0 = 0;
  uint32_t la = 0;
  if (live) {
    s0 = A.start[read];
    la = reads_fit_len(s0, A.len[read], A.bytes, 32u * W);  // (what does not fit the instance counts as empty too)
  }

  // ---- quality ----
  uint32_t lq = la;
  if (A.cutoff) {  // (the same in every lane of the grid)
    int32_t carry = 0;
    bool stopped = false;
    TrmLow low = trm_low_none(la);
#pragma unroll
    for (int r = W / 2 - 1; r >= 0; --r) {
      const uint32_t t = 64u * r + lane;
      const bool in = t < la;
      int32_t incl = in ? trm_term(A.qual[s0 + t], A.cutoff) : 0;
#pragma unroll
      for (uint32_t o = 1; o < 64u; o <<= 1) incl = trm_scan_add(incl, __shfl_down(incl, o, 64), lane, o);
      const int32_t s = carry + incl;
      const unsigned long long pos = __ballot(in & (s > 0));
      low = trm_low_take(low, s, t, in & !stopped & ((int32_t)lane > trm_stop_lane(pos)));
      stopped |= pos != 0ull;
      carry += __shfl(incl, 0, 64);
    }
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
      TrmLow other;
      other.s = __shfl_xor(low.s, step, 64);
      other.i = __shfl_xor(low.i, step, 64);
      low = trm_low_combine(low, other);
    }
    lq = trm_quality_len(low, la);
  }

  // ---- planes ----
  for (uint32_t i = lane; i < (uint32_t)(P + 1) * kTrmPad; i += 64u) planes[(i / kTrmPad) * S + W + i % kTrmPad] = 0u;
#pragma unroll
  for (int c = 0; c < W / 2; ++c) {
    const uint32_t t = 64u * c + lane;
    const uint32_t code = t < la ? pairs_row_code(profile, A.text[s0 + t]) : 0u;
#pragma unroll
    for (int p = 0; p <= P; ++p) {
      const unsigned long long w = __ballot(p == P ? t < lq : ((code >> p) & 1u) != 0u);
      if (lane < 2u) planes[p * S + 2 * c + lane] = lane ? (uint32_t)(w >> 32) : (uint32_t)w;
    }
  }
  __syncthreads();  // (every wavefront of the workgroup comes here, with or without a read)

  // ---- positions ----
  const uint32_t count = trm_positions(lq, A.min_overlap);
  TrmBest best = trm_none();
  for (uint32_t round = 0; round < ovl_rounds(count); ++round) {
    const uint32_t c_mine = round * kOvlWave + lane;
    const bool in_range = c_mine < count;
    const uint32_t c = in_range ? c_mine : count - 1u;  // (a lane past the last position repeats it and counts nothing)
    uint32_t rw[P + 1][2];
#pragma unroll
    for (int p = 0; p <= P; ++p) trm_window(planes + p * S, c, rw[p]);
    for (uint32_t j = 0; j < A.n_adapters; ++j) {
      const uint32_t* ad = A.tab + j * kTrmTableWords;
      const uint32_t mm = trm_mismatches<P, IUPAC>(rw, ad), ov = trm_overlap(ad[kTrmLenWord], lq, c);
      best = trm_combine(best, trm_one(c, ov, mm, j, in_range & ovl_accepts(mm, ov, A.min_overlap, A.k, A.max_permille)));
    }
    if (__ballot(best.found != 0u) != 0ull) break;  // (the same in every lane: a later round holds larger positions only)
  }

  // ---- the wavefront's result ----
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) {
    TrmBest other;
    other.c = __shfl_xor(best.c, step, 64);
    other.ov = __shfl_xor(best.ov, step, 64);
    other.mm = __shfl_xor(best.mm, step, 64);
    other.j = __shfl_xor(best.j, step, 64);
    other.found = __shfl_xor(best.found, step, 64);
    best = trm_combine(best, other);
  }
  if (live && lane == 0u) A.out[read] = trm_record(best, lq, A.min_length);
}

template <bool IUPAC>
hipError_t launch_words(uint32_t W, const TrimArgs& A, hipStream_t st) {
  const dim3 grid((uint32_t)((A.n + kTrmReadsPerGroup - 1) / kTrmReadsPerGroup)), block(64 * kTrmReadsPerGroup);
  // ovl_words: reads of at most 64, 128, 192, 256, 512 bytes
  if (W == 2) hipLaunchKernelGGL((trim_find_kernel<2, IUPAC>), grid, block, 0, st, A);
  else if (W == 4) hipLaunchKernelGGL((trim_find_kernel<4, IUPAC>), grid, block, 0, st, A);
  else if (W == 6) hipLaunchKernelGGL((trim_find_kernel<6, IUPAC>), grid, block, 0, st, A);
  else if (W == 8) hipLaunchKernelGGL((trim_find_kernel<8, IUPAC>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((trim_find_kernel<16, IUPAC>), grid, block, 0, st, A);
  return hipGetLastError();
}

struct WindowArgs {
  const uint8_t *src_text, *src_qual;  // src_qual: null where the qualities are not kept
  const uint64_t* src_start;           // the source handle's starts
  const uint64_t* begin;               // per read of the new handle, on the device; null: every window begins its read
  const uint64_t* src;                 // GATHER: per read of the new handle its read of the source handle
  uint32_t n_src;                      // reads of the source handle
  uint64_t src_bytes;                  // the source handle's text size (a multiple of 64)
  const uint64_t* table;               // of the new handle: starts[n], then lens[n]
  uint32_t n;                          // reads of the new handle
  uint64_t n_blocks;                   // of the new layout; block n_blocks is the spare one
  uint8_t *text, *qual;
  uint32_t* rem;
};

// SHIFTED: the windows begin anywhere in their reads (a slice).  Otherwise every window begins its read (a trim: A.begin is
// null), a read starts at a multiple of 64 and so does the block within it: four aligned loads, no shift.  GATHER: read t of
// the output is a window of read src[t] of the source (a select, a demux); otherwise t is its own source.
template <bool SHIFTED, bool GATHER>
__global__ __launch_bounds__(256) void reads_window_write_kernel(WindowArgs A) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > A.n_blocks) return;
  uint4* dst_t = reinterpret_cast<uint4*>(A.text + b * 64);
  uint4* dst_q = A.qual ? reinterpret_cast<uint4*>(A.qual + b * 64) : nullptr;
  if (b == A.n_blocks) {  // the spare bytes behind the layout
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dst_t[j] = make_uint4(0u, 0u, 0u, 0u);
      if (A.qual) dst_q[j] = make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }
  const uint32_t t = ham_text_of([&](uint32_t i) { return A.table[i]; }, A.n, b * 64);
  const uint64_t start = A.table[t];
  const uint32_t left = ham_rem(b, start, A.table[(uint64_t)A.n + t]);
  A.rem[b] = left;
  uint64_t from = t;
  if constexpr (GATHER) from = min(A.src[t], (uint64_t)A.n_src - 1u);  // (the host checked a select's table; a demux's is a permutation)
  const uint64_t src = A.src_start[from] + (SHIFTED ? A.begin[t] : 0ull) + (b * 64 - start);
  const uint32_t keep = min(left, 64u);
  TrmLoad16 load16{A.src_text};
  if constexpr (SHIFTED) {
    uint32_t out[16];
    trm_window_block(load16, src, A.src_bytes, keep, out);
#pragma unroll
    for (int j = 0; j < 4; ++j) dst_t[j] = make_uint4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
    if (A.qual) {
      load16.base = A.src_qual;
      trm_window_block(load16, src, A.src_bytes, keep, out);
#pragma unroll
      for (int j = 0; j < 4; ++j) dst_q[j] = make_uint4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
    }
  } else {  // every load of the block first, then the stores: sixteen words of text and sixteen of quality in flight at once
    uint32_t wt[4][4], wq[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) trm_aligned_quarter(load16, src, A.src_bytes, keep, q, wt[q]);
    if (A.qual) {
      load16.base = A.src_qual;
#pragma unroll
      for (int q = 0; q < 4; ++q) trm_aligned_quarter(load16, src, A.src_bytes, keep, q, wq[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) dst_t[q] = make_uint4(wt[q][0], wt[q][1], wt[q][2], wt[q][3]);
    if (A.qual) {
#pragma unroll
      for (int q = 0; q < 4; ++q) dst_q[q] = make_uint4(wq[q][0], wq[q][1], wq[q][2], wq[q][3]);
    }
  }
}

}  // namespace

// a handle without a record or without a byte: the 64 spare bytes of its buffers
int reads_empty_buffers(sassy_hip_Reads* F, bool keep_quality, hipStream_t st) {
  F->text_bytes = 64;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&F->d_text), 64));
  HIP_TRY(hipMemsetAsync(F->d_text, 0, 64, st));
  if (keep_quality) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&F->d_qual), 64));
    HIP_TRY(hipMemsetAsync(F->d_qual, 0, 64, st));
  }
  return 0;
}

// the write kernel over a laid-out handle F whose read r is a window of read r of `reads`, or of read d_src[r] where that
// table is given (n_records of F entries, each below n_records of `reads`, which then holds a read)
int write_windows(const sassy_hip_Reads* reads, const uint64_t* d_src, const uint64_t* d_begin, sassy_hip_Reads* F, hipStream_t st) {
  WindowArgs A;
  A.src_text = reads->d_text; A.src_qual = F->d_qual ? reads->d_qual : nullptr;
  A.src_start = reads->d_table; A.begin = d_begin;
  A.src = d_src; A.n_src = (uint32_t)reads->n_records;
  A.src_bytes = reads->text_bytes;
  A.table = F->d_table;
  A.n = (uint32_t)F->n_records;
  A.n_blocks = (F->text_bytes - 64) / 64;
  A.text = F->d_text; A.qual = F->d_qual; A.rem = F->d_rem;
  const dim3 grid((uint32_t)((A.n_blocks + 1 + 255) / 256));
  if (d_src && d_begin) hipLaunchKernelGGL((reads_window_write_kernel<true, true>), grid, dim3(256), 0, st, A);
  else if (d_src) hipLaunchKernelGGL((reads_window_write_kernel<false, true>), grid, dim3(256), 0, st, A);
  else if (d_begin) hipLaunchKernelGGL((reads_window_write_kernel<true, false>), grid, dim3(256), 0, st, A);
  else hipLaunchKernelGGL((reads_window_write_kernel<false, false>), grid, dim3(256), 0, st, A);
  HIP_TRY(hipGetLastError());
  return 0;
}

namespace {

// what a refusal of the call's own checks says
std::string refusal_text(TrmRefusal why, const TrmCall& c, size_t which) {
  const std::string a = "trim_reads: adapter " + std::to_string(which);
  if (why == kTrmNullSearcher) return "Pointers in trim_reads() must not be null";
  if (why == kTrmFlags) return "trim_reads takes no flags (the read batch is on the device)";
  if (why == kTrmMinOverlap) return "trim_reads: min_overlap must be at least 1";
  if (why == kTrmPermille) return "trim_reads: max_permille must be <= 1000 (got " + std::to_string(c.max_permille) + ")";
  if (why == kTrmCutoff) return "trim_reads: quality_cutoff must be <= 93 (Phred+33; got " + std::to_string(c.quality_cutoff) + ")";
  if (why == kTrmTooMany)
    return "trim_reads takes at most " + std::to_string(kTrmMaxAdapters) + " adapters (SASSY_HIP_TRIM_MAX_ADAPTERS; got " + std::to_string(c.n_adapters) + ")";
  if (why == kTrmNullAdapter) return "Pointers in trim_reads() must not be null (adapter " + std::to_string(which) + ")";
  if (why == kTrmEmptyAdapter) return a + " is empty";
  if (why == kTrmLongAdapter)
    return a + " has " + std::to_string(c.adapter_lens[which]) + " bytes: an adapter has at most " + std::to_string(kTrmMaxAdapterLen);
  if (why == kTrmShortAdapter)
    return a + " has " + std::to_string(c.adapter_lens[which]) + " bytes, fewer than min_overlap = " + std::to_string(c.min_overlap) + ": it could never be accepted";
  if (why == kTrmNoQuality) return "trim_reads: the reads were parsed without SASSY_HIP_KEEP_QUALITY: quality_cutoff needs the base qualities";
  if (why == kTrmNullTrimmed) return "Pointers in trim_reads() must not be null (out_trimmed)";
  return "trim_reads: refused";
}

// The call behind its refusals, inside reads_new_batch (the device, fresh stats, k cut to the longest adapter, the fresh handle F).
int trim_run(sassy_SearcherType* s, const sassy_hip_Reads* reads, const uint8_t* const* adapters, const size_t* adapter_lens, size_t n_adapters,
             uint32_t min_overlap, uint32_t k, uint32_t max_permille, uint32_t cutoff, uint32_t min_length, sassy_hip_ReadTrim* out_trims,
             sassy_hip_Reads* F) {
  hipStream_t st = s->stream;
  const uint64_t n = reads->n_records;
  const bool keep_quality = reads->d_qual != nullptr;
  if (s->profile == PROFILE_DNA)  // the 2-bit codes are exact on A, C, G, T only: the adapters first, whatever the batch holds
    for (size_t j = 0; j < n_adapters; ++j)
      if (!acgt_only(adapters[j], adapter_lens[j]))
        return fail(SASSY_HIP_EINVAL, "trim_reads: adapter " + std::to_string(j) + " holds other bytes than A, C, G, T: use an iupac searcher");
  if (n == 0) {
    if (int rc = reads_empty_buffers(F, keep_quality, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  const uint32_t profile = s->profile == PROFILE_IUPAC ? kHamIupac : kHamDna;
  uint32_t launches = 5;  // the find kernel, the three kernels of the layout scan, the write kernel; the Dna look where it runs
  if (int rc = reads_require_plain(s, reads, "trim_reads", "the reads hold", "encode", &launches)) return rc;
  if ((n + kTrmReadsPerGroup - 1) / kTrmReadsPerGroup > 0x7FFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "trim_reads: too many reads for a grid");
  std::vector<uint32_t> tab(std::max<size_t>(n_adapters, 1) * kTrmTableWords, 0u);
  for (size_t j = 0; j < n_adapters; ++j) trm_encode_adapter(profile, adapters[j], (uint32_t)adapter_lens[j], tab.data() + j * kTrmTableWords);
  if (int rc = s->d_trim_tab.reserve(tab.size())) return rc;
  if (int rc = s->d_trims.reserve(n)) return rc;
  HIP_TRY(hipMemcpyAsync(s->d_trim_tab.p, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  TrimArgs A;
  A.text = reads->d_text; A.qual = reads->d_qual;
  A.start = reads->d_table; A.len = reads->d_table + n;
  A.bytes = reads->text_bytes;
  A.n = n;
  A.tab = s->d_trim_tab.p;
  A.n_adapters = (uint32_t)n_adapters; A.min_overlap = min_overlap;
  A.k = k;
  A.max_permille = max_permille; A.cutoff = cutoff; A.min_length = min_length;
  A.out = reinterpret_cast<TrmRecord*>(s->d_trims.p);
  const uint32_t W = ovl_words((uint32_t)reads->longest);
  if (s->timing >= 1) HIP_TRY(hipEventRecord(s->ev_line[0], st));
  HIP_TRY(s->profile == PROFILE_IUPAC ? launch_words<true>(W, A, st) : launch_words<false>(W, A, st));
  if (s->timing >= 1) HIP_TRY(hipEventRecord(s->ev_line[1], st));
  uint64_t n_found = 0;
  if (int rc = reads_layout_trimmed(s->d_trims.p, n, keep_quality, &s->lanes[0], F, &n_found)) return rc;  // (waits: `tab` has landed)
  if (int rc = write_windows(reads, nullptr, nullptr, F, st)) return rc;
  if (out_trims)
    if (int rc = s->lanes[0].download(out_trims, s->d_trims.p, n * sizeof(sassy_hip_ReadTrim))) return rc;
  HIP_TRY(hipStreamSynchronize(st));  // (the handle is whole when the call returns, and the records are free again)
  if (s->timing >= 1) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, s->ev_line[0], s->ev_line[1]);
    s->stats.scan_ms = ms;
  }
  s->stats.scan_launches = launches;
  s->stats.candidates = n_found;
  s->stats.blocks = (n + kTrmReadsPerGroup - 1) / kTrmReadsPerGroup;
  s->stats.word_rows = W;
  s->stats.text_bytes = reads->text_bytes - 64;
  return 0;
}

}  // namespace
}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_trim_reads(sassy_SearcherType* s, const sassy_hip_Reads* reads, const uint8_t* const* adapters, const size_t* adapter_lens,
                         size_t n_adapters, uint32_t min_overlap, size_t k, uint32_t max_permille, uint32_t quality_cutoff, uint32_t min_length,
                         uint32_t flags, sassy_hip_ReadTrim* out_trims, sassy_hip_Reads** out_trimmed) {
  if (out_trimmed) *out_trimmed = nullptr;
  TrmCall c{};
  c.have_searcher = s != nullptr; c.have_trimmed = out_trimmed != nullptr;
  c.flags = flags; c.min_overlap = min_overlap; c.max_permille = max_permille; c.quality_cutoff = quality_cutoff;
  c.adapters = adapters; c.adapter_lens = adapter_lens; c.n_adapters = n_adapters;
  c.gate = reads_gate_of(s, 1, reads, nullptr);
  // the searcher, the numbers and the adapters first: the batch is read only once nothing in front of it is wrong
  size_t which = 0;
  ReadsRefusal gate = kRdsOk;
  TrmRefusal why = trm_refusal(c, &which, &gate);
  if (why == kTrmOk || why == kTrmNullTrimmed || (why == kTrmGate && gate == kRdsInFlight)) {
    reads_gate_read(s, reads, nullptr, &c.gate);
    c.kept_quality = reads->d_qual != nullptr;
    why = trm_refusal(c, &which, &gate);
  }
  if (why == kTrmGate)
    return reads_refused(gate, c.gate, ReadsWho{"trim_reads", "adapters are DNA", "scores the adapter's overlap with the read's end itself",
                                                "reports the best position of every read"});
  if (why != kTrmOk) return fail(SASSY_HIP_EINVAL, refusal_text(why, c, which));
  return reads_new_batch(s, kTrmMaxAdapterLen, k, out_trimmed, [&](uint32_t kk, sassy_hip_Reads* F) {  // (k beyond the longest adapter accepts what k == 64 does)
    return trim_run(s, reads, adapters, adapter_lens, n_adapters, min_overlap, kk, max_permille, quality_cutoff, min_length, out_trims, F);
  });
}

int sassy_hip_reads_slice(const sassy_hip_Reads* reads, const uint64_t* begins, const uint64_t* lens, void* hip_stream, sassy_hip_Reads** out) {
  if (out) *out = nullptr;
  if (!reads || !out || (reads->n_records && (!begins || !lens))) return fail(SASSY_HIP_EINVAL, "Pointers in reads_slice() must not be null");
  for (uint64_t r = 0; r < reads->n_records; ++r) {
    const uint64_t have = reads->records[r].seq_len;
    if (begins[r] > have || lens[r] > have - begins[r])
      return fail(SASSY_HIP_EINVAL, "reads_slice: window " + std::to_string(r) + " [" + std::to_string(begins[r]) + ", +" + std::to_string(lens[r]) +
                                        ") reaches outside its read of " + std::to_string(have) + " bytes");
  }
  return windows_from_host(reads, nullptr, begins, lens, reads->n_records, reinterpret_cast<hipStream_t>(hip_stream), "reads_slice", out);
}

}  // extern "C"
