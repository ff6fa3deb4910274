// demux_reads.hip -- a resident read batch split by sample barcode into a NEW resident read batch whose records are sorted by
// sample, the barcode clipped off (sassy_hip_demux_reads), and the gather that makes a batch out of any
// reads of another in any order (sassy_hip_reads_select).  The arithmetic -- the refusals, the window, the planes, the
// mismatches of a barcode, best / second / n_best, the assignment, the clip, the record, the bounds -- is demux_step.h's; a
// block of a window is trim_step.h's; the layout rule and its scan are the parse's (fastq_reads.hip: reads_layout_windows);
// the write kernel is the trim's (trim_reads.hip: write_windows).
//
// Device work of a demux, all on the searcher's stream:
//   demux_assign_kernel   a lane per read.  The read's window (at most 64 bytes at any alignment) as five 16-byte pieces
//              through trm_window_block, bounded by the handle's text size; its bytes packed into two words per plane; then
//              the loop over the barcodes, whose table entry is wave-uniform (scalar loads): xor / and / or, one 64-bit
//              popcount, dmx_combine.  One 16-byte store of the record, the label and the read's index as the sort's pair.
//   rocPRIM radix sort    (label, read index), stable, over the bits of B.
//   demux_bounds_kernel   a lane per label: its first place in the sorted labels, by lower bound.
//   demux_place_kernel    a lane per output record: `index` into its read's record, the order as 64-bit entries, begin, len.
//   fastq_rec_sum / _top / _write_kernel    the layout from the table of lengths  -> host (one wait)
//   reads_window_write_kernel<.., GATHER>   the trim's, record j from read order[j]: shifted for a clip at the 5' end, aligned
//              otherwise.
// The input handle is only read.  Every load of a read's bytes is bounded by the handle's length table and its text size,
// every store by the read count, the label count or the block count.
#include <hip/hip_runtime.h>

#include <cstring>  // (rocprim's texture iterator uses memset without including it)

#include <rocprim/rocprim.hpp>

#include "host_internal.h"
#include "fastq_step.h"
#include "hamming_step.h"
#include "demux_step.h"

static_assert(sizeof(sassy_hip_ReadDemux) == 16 && sizeof(sassy_hip::DmxRecord) == 16, "one 16-byte store per read");
static_assert(offsetof(sassy_hip_ReadDemux, cost) == 8 && offsetof(sassy_hip_ReadDemux, second) == 9 && offsetof(sassy_hip_ReadDemux, n_best) == 10 &&
                  offsetof(sassy_hip_ReadDemux, index) == 12,
              "DmxRecord::tail is the record's third word");
static_assert(SASSY_HIP_DEMUX_MAX_BARCODES == sassy_hip::kDmxMaxBarcodes && SASSY_HIP_DEMUX_END3 == sassy_hip::kDmxEnd3 &&
                  SASSY_HIP_DEMUX_KEEP_BARCODE == sassy_hip::kDmxKeepBarcode,
              "the header's numbers are the step header's");

namespace sassy_hip {
namespace {

struct AssignArgs {
  const uint8_t* text;
  const uint64_t *start, *len;  // the handle's tables
  uint64_t bytes;               // the handle's text size
  uint64_t n;
  const uint32_t* tab;          // n_barcodes entries of dmx_entry_words words
  uint32_t n_barcodes, m, at, end3, k, min_delta;
  DmxRecord* rec;
  uint32_t *label, *idx;        // the sort's keys and values
};

template <bool IUPAC>
__global__ __launch_bounds__(256) void demux_assign_kernel(AssignArgs A) {
  constexpr int P = IUPAC ? 4 : 2;
  constexpr uint32_t profile = IUPAC ? kHamIupac : kHamDna;
  const uint64_t read = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = read < A.n;
  uint64_t s0 = 0;
  uint32_t la = 0;
  if (live) {
    s0 = A.start[read];
    la = reads_fit_len(s0, A.len[read], A.bytes, kOvlMaxLen);
  }
  const bool has_window = live & dmx_has_window(la, A.at, A.m);

  // ---- the window and its planes ----
  uint32_t blk[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) blk[j] = 0u;
  if (has_window) {
    trm_window_block(TrmLoad16{A.text}, s0 + dmx_window(la, A.at, A.m, A.end3 != 0u), A.bytes, A.m, blk);
  }
  uint32_t rw[P + 1][2];
  dmx_planes<P>(profile, blk, rw);

  // ---- the barcodes: the entry is the same in every lane ----
  const uint32_t mask[2] = {dmx_row_mask(A.m, 0), dmx_row_mask(A.m, 1)};
  DmxBest best = dmx_none();
  for (uint32_t j = 0; j < A.n_barcodes; ++j)
    best = dmx_combine(best, dmx_one(dmx_mismatches<P, IUPAC>(rw, A.tab + (uint64_t)j * (2 * P), mask), j, A.m));

  if (live) {
    const bool assigned = dmx_assigned(has_window, best, A.k, A.min_delta);
    A.rec[read] = dmx_record(has_window, assigned, best);
    A.label[read] = dmx_label(assigned, best, A.n_barcodes);
    A.idx[read] = (uint32_t)read;
  }
}

// bounds[s], s = 0 .. n_labels: the first place of label s among the sorted labels (n_labels = B + 1, so bounds has B + 2)
__global__ __launch_bounds__(256) void demux_bounds_kernel(const uint32_t* sorted, uint64_t n, uint32_t n_labels, uint64_t* bounds) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > n_labels) return;
  bounds[s] = dmx_lower_bound([&](uint64_t i) { return sorted[i]; }, n, s);
}

struct PlaceArgs {
  const uint32_t* sorted_idx;  // the order
  const uint64_t* len;         // the source handle's lengths
  uint64_t n;
  uint32_t m, at, end3, keep_barcode;
  DmxRecord* rec;
  uint64_t *order, *begin, *out_len;
};
__global__ __launch_bounds__(256) void demux_place_kernel(PlaceArgs A) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.n) return;
  const uint64_t r = min((uint64_t)A.sorted_idx[j], A.n - 1);  // (a permutation of 0 .. n - 1)
  DmxRecord* R = A.rec + r;
  R->index = (uint32_t)j;
  const uint32_t la = (uint32_t)min(A.len[r], (uint64_t)kOvlMaxLen);
  const bool assigned = R->sample != 0xFFFFFFFFu && dmx_has_window(la, A.at, A.m);  // (an assigned read has a window)
  const DmxClip c = dmx_clip(la, A.at, A.m, A.end3 != 0u, A.keep_barcode != 0u, assigned);
  A.order[j] = r;
  A.begin[j] = c.begin;
  A.out_len[j] = c.len;
}

// what a refusal of the call's own checks says
std::string refusal_text(DmxRefusal why, const DmxCall& c, size_t which) {
  if (why == kDmxNullSearcher) return "Pointers in demux_reads() must not be null";
  if (why == kDmxFlags) return "demux_reads takes SASSY_HIP_DEMUX_END3 and SASSY_HIP_DEMUX_KEEP_BARCODE only (the read batch is on the device)";
  if (why == kDmxDelta) return "demux_reads: min_delta must be <= " + std::to_string(kDmxMaxDelta) + " (got " + std::to_string(c.min_delta) + ")";
  if (why == kDmxCount)
    return "demux_reads takes 1 .. " + std::to_string(kDmxMaxBarcodes) + " barcodes (SASSY_HIP_DEMUX_MAX_BARCODES; got " + std::to_string(c.n_barcodes) + ")";
  if (why == kDmxLen) return "demux_reads: barcode_len must be 1 .. " + std::to_string(kDmxMaxLen) + " (got " + std::to_string(c.barcode_len) + ")";
  if (why == kDmxNullBarcode) return "Pointers in demux_reads() must not be null (barcode " + std::to_string(which) + ")";
  if (why == kDmxAt)
    return "demux_reads: at + barcode_len = " + std::to_string((uint64_t)c.at + c.barcode_len) + " reaches past the longest read a batch may hold (" +
           std::to_string(kOvlMaxLen) + ")";
  if (why == kDmxNullOut) return "Pointers in demux_reads() must not be null (out_bounds, out_sorted)";
  return "demux_reads: refused";
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// The call behind its refusals, inside reads_new_batch (the device, fresh stats, k cut to the longest barcode, the fresh handle F).
int demux_run(sassy_SearcherType* s, const sassy_hip_Reads* reads, const uint8_t* const* barcodes, uint32_t m, uint32_t B, uint32_t at, uint32_t k,
              uint32_t min_delta, uint32_t flags, sassy_hip_ReadDemux* out_assign, uint64_t* out_order, uint64_t* out_bounds, sassy_hip_Reads* F) {
  hipStream_t st = s->stream;
  const uint64_t n = reads->n_records;
  const bool keep_quality = reads->d_qual != nullptr;
  if (s->profile == PROFILE_DNA)  // the 2-bit codes are exact on A, C, G, T only: the barcodes first, whatever the batch holds
    for (uint32_t j = 0; j < B; ++j)
      if (!acgt_only(barcodes[j], m))
        return fail(SASSY_HIP_EINVAL, "demux_reads: barcode " + std::to_string(j) + " holds other bytes than A, C, G, T: use an iupac searcher");
  for (uint32_t i = 0; i < B + 2; ++i) out_bounds[i] = 0;
  if (n == 0) {
    if (int rc = reads_empty_buffers(F, keep_quality, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  const uint32_t profile = s->profile == PROFILE_IUPAC ? kHamIupac : kHamDna;
  // the assign kernel, the sort (the library's launches count as one), the bounds and the place kernel, the three kernels of the
  // layout scan, the write kernel; the Dna look where it runs
  uint32_t launches = 8;
  if (int rc = reads_require_plain(s, reads, "demux_reads", "the reads hold", "encode", &launches)) return rc;
  const uint32_t E = dmx_entry_words(profile);
  std::vector<uint32_t> tab((size_t)B * E, 0u);
  for (uint32_t j = 0; j < B; ++j) dmx_encode_barcode(profile, barcodes[j], m, tab.data() + (size_t)j * E);
  const unsigned bits = dmx_key_bits(B);
  size_t temp_bytes = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                    static_cast<uint32_t*>(nullptr), (size_t)n, 0u, bits, st));
  // one area: the records, the keys and values of the sort twice, the order, the begins, the lengths, the bounds, the sort's own
  const size_t o_rec = 0, o_key = o_rec + up256(n * 16), o_key2 = o_key + up256(n * 4), o_idx = o_key2 + up256(n * 4), o_idx2 = o_idx + up256(n * 4),
               o_order = o_idx2 + up256(n * 4), o_begin = o_order + up256(n * 8), o_len = o_begin + up256(n * 8), o_bounds = o_len + up256(n * 8),
               o_temp = o_bounds + up256(((size_t)B + 2) * 8), total = o_temp + up256(temp_bytes);
  if (int rc = s->d_demux_tab.reserve(tab.size())) return rc;
  if (int rc = s->d_demux.reserve(total)) return rc;
  uint8_t* base = s->d_demux.p;
  DmxRecord* d_rec = reinterpret_cast<DmxRecord*>(base + o_rec);
  uint32_t *d_key = reinterpret_cast<uint32_t*>(base + o_key), *d_key2 = reinterpret_cast<uint32_t*>(base + o_key2);
  uint32_t *d_idx = reinterpret_cast<uint32_t*>(base + o_idx), *d_idx2 = reinterpret_cast<uint32_t*>(base + o_idx2);
  uint64_t *d_order = reinterpret_cast<uint64_t*>(base + o_order), *d_begin = reinterpret_cast<uint64_t*>(base + o_begin);
  uint64_t *d_len = reinterpret_cast<uint64_t*>(base + o_len), *d_bounds = reinterpret_cast<uint64_t*>(base + o_bounds);
  HIP_TRY(hipMemcpyAsync(s->d_demux_tab.p, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));

  AssignArgs A;
  A.text = reads->d_text;
  A.start = reads->d_table; A.len = reads->d_table + n;
  A.bytes = reads->text_bytes;
  A.n = n;
  A.tab = s->d_demux_tab.p;
  A.n_barcodes = B; A.m = m; A.at = at; A.end3 = (flags & kDmxEnd3) ? 1u : 0u;
  A.k = k;
  A.min_delta = min_delta;
  A.rec = d_rec; A.label = d_key; A.idx = d_idx;
  const dim3 per_read((uint32_t)((n + 255) / 256)), block(256);
  if (s->timing >= 1) HIP_TRY(hipEventRecord(s->ev_line[0], st));
  if (s->profile == PROFILE_IUPAC) hipLaunchKernelGGL(demux_assign_kernel<true>, per_read, block, 0, st, A);
  else hipLaunchKernelGGL(demux_assign_kernel<false>, per_read, block, 0, st, A);
  HIP_TRY(hipGetLastError());
  if (s->timing >= 1) HIP_TRY(hipEventRecord(s->ev_line[1], st));
  HIP_TRY(rocprim::radix_sort_pairs(base + o_temp, temp_bytes, d_key, d_key2, d_idx, d_idx2, (size_t)n, 0u, bits, st));
  hipLaunchKernelGGL(demux_bounds_kernel, dim3((B + 2 + 255) / 256), block, 0, st, (const uint32_t*)d_key2, n, B + 1, d_bounds);
  HIP_TRY(hipGetLastError());
  PlaceArgs Pl;
  Pl.sorted_idx = d_idx2; Pl.len = reads->d_table + n; Pl.n = n;
  Pl.m = m; Pl.at = at; Pl.end3 = A.end3; Pl.keep_barcode = (flags & kDmxKeepBarcode) ? 1u : 0u;
  Pl.rec = d_rec; Pl.order = d_order; Pl.begin = d_begin; Pl.out_len = d_len;
  hipLaunchKernelGGL(demux_place_kernel, per_read, block, 0, st, Pl);
  HIP_TRY(hipGetLastError());
  if (int rc = reads_layout_windows(d_len, n, keep_quality, st, F)) return rc;  // (waits: `tab` has landed)
  if (int rc = write_windows(reads, d_order, dmx_shifted(flags) ? d_begin : nullptr, F, st)) return rc;
  if (int rc = s->lanes[0].download(out_bounds, d_bounds, ((size_t)B + 2) * sizeof(uint64_t))) return rc;
  if (out_assign)
    if (int rc = s->lanes[0].download(out_assign, d_rec, n * sizeof(sassy_hip_ReadDemux))) return rc;
  if (out_order)
    if (int rc = s->lanes[0].download(out_order, d_order, n * sizeof(uint64_t))) return rc;
  HIP_TRY(hipStreamSynchronize(st));  // (the handle is whole when the call returns, and the area is free again)
  if (s->timing >= 1) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, s->ev_line[0], s->ev_line[1]);
    s->stats.scan_ms = ms;
  }
  s->stats.scan_launches = launches;
  s->stats.candidates = out_bounds[B];
  s->stats.blocks = (n + 255) / 256;
  s->stats.word_rows = 2;
  s->stats.text_bytes = reads->text_bytes - 64;
  return 0;
}

}  // namespace
}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_demux_reads(sassy_SearcherType* s, const sassy_hip_Reads* reads, const uint8_t* const* barcodes, size_t barcode_len, size_t n_barcodes,
                          uint32_t at, size_t k, uint32_t min_delta, uint32_t flags, sassy_hip_ReadDemux* out_assign, uint64_t* out_order,
                          uint64_t* out_bounds, sassy_hip_Reads** out_sorted) {
  if (out_sorted) *out_sorted = nullptr;
  DmxCall c{};
  c.have_searcher = s != nullptr; c.have_bounds = out_bounds != nullptr; c.have_sorted = out_sorted != nullptr;
  c.flags = flags; c.min_delta = min_delta; c.at = at;
  c.n_barcodes = n_barcodes; c.barcode_len = barcode_len; c.barcodes = barcodes;
  c.gate = reads_gate_of(s, 1, reads, nullptr);
  // the searcher, the numbers and the barcodes first: the batch is read only once nothing in front of it is wrong
  size_t which = 0;
  ReadsRefusal gate = kRdsOk;
  DmxRefusal why = dmx_refusal(c, &which, &gate);
  if (why == kDmxOk || why == kDmxNullOut || (why == kDmxGate && gate == kRdsInFlight)) {
    reads_gate_read(s, reads, nullptr, &c.gate);
    why = dmx_refusal(c, &which, &gate);
  }
  if (why == kDmxGate)
    return reads_refused(gate, c.gate, ReadsWho{"demux_reads", "barcodes are DNA", "compares the barcode with a window that lies inside the read",
                                                "reports the best barcode of every read"});
  if (why != kDmxOk) return fail(SASSY_HIP_EINVAL, refusal_text(why, c, which));
  return reads_new_batch(s, kDmxMaxLen, k, out_sorted, [&](uint32_t kk, sassy_hip_Reads* F) {  // (k beyond the longest barcode accepts what k == 64 does)
    return demux_run(s, reads, barcodes, (uint32_t)barcode_len, (uint32_t)n_barcodes, at, kk, min_delta, flags, out_assign, out_order, out_bounds, F);
  });
}

int sassy_hip_reads_select(const sassy_hip_Reads* reads, const uint64_t* src, const uint64_t* begins, const uint64_t* lens, uint64_t n_out,
                           void* hip_stream, sassy_hip_Reads** out) {
  if (out) *out = nullptr;
  if (!reads || !out || (n_out && !src)) return fail(SASSY_HIP_EINVAL, "Pointers in reads_select() must not be null");
  if ((begins == nullptr) != (lens == nullptr)) return fail(SASSY_HIP_EINVAL, "reads_select: begins and lens are given together, or both NULL (whole reads)");
  if (n_out > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "reads_select: " + std::to_string(n_out) + " records, more than 2^32 - 1");
  for (uint64_t j = 0; j < n_out; ++j) {
    if (src[j] >= reads->n_records)
      return fail(SASSY_HIP_EINVAL, "reads_select: src " + std::to_string(j) + " = " + std::to_string(src[j]) + " names no read of a batch of " +
                                        std::to_string(reads->n_records));
    const uint64_t have = reads->records[src[j]].seq_len;
    if (begins && (begins[j] > have || lens[j] > have - begins[j]))
      return fail(SASSY_HIP_EINVAL, "reads_select: window " + std::to_string(j) + " [" + std::to_string(begins[j]) + ", +" + std::to_string(lens[j]) +
                                        ") reaches outside its read of " + std::to_string(have) + " bytes");
  }
  return windows_from_host(reads, src, begins, lens, n_out, reinterpret_cast<hipStream_t>(hip_stream), "reads_select", out);
}

}  // extern "C"
