// merge_pairs.hip -- every pair of two resident read batches that has an accepted overlap, merged into a NEW resident read
// batch with consensus sequence and consensus quality (sassy_hip_merge_pairs).  Record r of the result is the
// merged read of pair r, empty where the pair was not merged, so an index means the same pair in all three handles.  The
// arithmetic -- the refusals, the merged length, what covers a column, the consensus -- is merge_step.h's; the overlap is
// read_overlaps.hip's kernel (overlaps_resident), whose records stay on the device; the layout rule and its scan are the
// parse's (fastq_reads.hip: reads_layout_merged).
//
// Device work, all on the searcher's stream:
//   read_overlaps_kernel                    the records, s->d_overlaps
//   fastq_rec_sum / _top / _write_kernel    L per pair from the records, starts = the exclusive scan of L rounded up to 64,
//                                           the record table, the longest merged read, the layout's size  -> host (one wait)
//   merge_write_kernel   a lane per 64-byte block of the OUTPUT, as fastq_copy_kernel: a million 12-base merges and a thousand
//                        1 000-base merges load the machine alike.  The block's pair by ham_text_of over the merged starts;
//                        R2's 64 bytes lie at any alignment and come as five 16-byte loads shifted by fq_shift_block, then
//                        word-reversed; a's 64 bytes and qualities are aligned 16-byte loads (a read starts at a multiple of
//                        64, and so does the block within it), taken a quarter at a time; the consensus word by word
//                        (mrg_word); four 16-byte stores each into the text and the quality buffer, each as its quarter is
//                        made, zeros behind the read's end, rem[block]; one extra lane zeroes the 64 spare bytes of both.
//                        Neither buffer is cleared as a whole.
// The input handles are only read.  Every load of a read's bytes is bounded by the handle's length table and its text size,
// every store by the block count.
#include <hip/hip_runtime.h>

#include "host_internal.h"
#include "fastq_step.h"
#include "hamming_step.h"
#include "merge_step.h"

namespace sassy_hip {
namespace {

struct MergeArgs {
  const uint8_t *text1, *qual1, *text2, *qual2;
  const uint64_t *start1, *len1, *start2, *len2;  // the input handles' tables
  uint64_t bytes1, bytes2;                        // the input handles' text sizes (multiples of 64)
  const sassy_hip_ReadOverlap* rec;
  const uint64_t* table;  // of the merged handle: starts[n], then lens[n]
  uint32_t n;
  uint64_t n_blocks;      // of the merged layout; block n_blocks is the spare one
  uint8_t *text, *qual;
  uint32_t* rem;
};

// four words at a 16-byte aligned address: a whole 16-byte piece, or zeros where it would begin at or behind `bytes`
__device__ __forceinline__ void load_aligned16(const uint8_t* base, uint64_t at, uint64_t bytes, uint32_t (&w)[4]) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (at < bytes) v = *reinterpret_cast<const uint4*>(base + at);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
// the 64 bytes from `src` on (any alignment, any sign: what lies in front of the buffer or behind `bytes` reads as zero)
__device__ __forceinline__ void load_shifted64(const uint8_t* base, int64_t src, uint64_t bytes, uint32_t (&out)[16]) {
  const int64_t al = src & ~(int64_t)15;
  uint32_t w[20];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int64_t at = al + 16 * j;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (at >= 0 && (uint64_t)at < bytes) v = *reinterpret_cast<const uint4*>(base + at);
    w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
  }
  fq_shift_block(w, (uint32_t)(src & 15), 64u, out);
}

template <bool IUPAC>
__global__ __launch_bounds__(256) void merge_write_kernel(MergeArgs A) {
  constexpr uint32_t profile = IUPAC ? kHamIupac : kHamDna;
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > A.n_blocks) return;
  uint4* dst_t = reinterpret_cast<uint4*>(A.text + b * 64);
  uint4* dst_q = reinterpret_cast<uint4*>(A.qual + b * 64);
  if (b == A.n_blocks) {  // the spare bytes behind the layout
#pragma unroll
    for (int j = 0; j < 4; ++j) dst_t[j] = dst_q[j] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const uint32_t t = ham_text_of([&](uint32_t i) { return A.table[i]; }, A.n, b * 64);
  const uint64_t start = A.table[t], merged_len = A.table[(uint64_t)A.n + t];
  A.rem[b] = ham_rem(b, start, merged_len);
  const uint32_t pb = (uint32_t)(b * 64 - start), len = (uint32_t)min(merged_len, (uint64_t)(2u * kOvlMaxLen));
  const sassy_hip_ReadOverlap rec = A.rec[t];
  const uint64_t s1 = A.start1[t], s2 = A.start2[t], l1 = A.len1[t], l2 = A.len2[t];
  // (as the overlap kernel: a pair that does not fit its texts counts as two empty reads)
  const bool fits = l1 <= kOvlMaxLen && l2 <= kOvlMaxLen && s1 <= A.bytes1 && l1 <= A.bytes1 - s1 && s2 <= A.bytes2 && l2 <= A.bytes2 - s2;
  const uint32_t la = fits ? (uint32_t)l1 : 0u, lb = fits ? (uint32_t)l2 : 0u;
  const uint64_t a_at = fits ? s1 + pb : A.bytes1;
  const int64_t b_at = fits ? (int64_t)s2 + mrg_r2_first(pb, lb, rec.offset) : -64;
  // b's block first, whole (the shift needs all of it); a's comes a quarter at a time and each quarter is stored as it is
  // made, so that a lane never holds a block of all four inputs and both outputs at once
  uint32_t wb[16], qb[16];
  load_shifted64(A.text2, b_at, A.bytes2, wb);
  load_shifted64(A.qual2, b_at, A.bytes2, qb);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t wa[4], qa[4], out_t[4], out_q[4];
    load_aligned16(A.text1, a_at + 16u * q, A.bytes1, wa);
    load_aligned16(A.qual1, a_at + 16u * q, A.bytes1, qa);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * q + i;
      const MrgWord w = mrg_word(profile, pb + 4u * j, la, lb, rec.offset, len, wa[i], qa[i], mrg_reverse_word(wb[15 - j]), mrg_reverse_word(qb[15 - j]));
      out_t[i] = w.text;
      out_q[i] = w.qual;
    }
    dst_t[q] = make_uint4(out_t[0], out_t[1], out_t[2], out_t[3]);
    dst_q[q] = make_uint4(out_q[0], out_q[1], out_q[2], out_q[3]);
  }
}

// The call behind its refusals, inside reads_new_batch (the device, fresh stats, k cut to the longest read, the fresh handle F).
int merge_run(sassy_SearcherType* s, const sassy_hip_Reads* r1, const sassy_hip_Reads* r2, uint32_t min_overlap, uint32_t k, uint32_t max_permille,
              sassy_hip_ReadOverlap* out_overlaps, sassy_hip_Reads* F) {
  hipStream_t st = s->stream;
  const uint64_t n = r1->n_records;
  if (n == 0) {  // no pair: the 64 spare bytes of both buffers
    if (int rc = reads_empty_buffers(F, true, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  if (int rc = overlaps_resident(s, r1, r2, min_overlap, k, max_permille, out_overlaps)) return rc;
  uint64_t n_merged = 0;
  if (int rc = reads_layout_merged(s->d_overlaps.p, r1->d_table + n, r2->d_table + n, n, &s->lanes[0], F, &n_merged)) return rc;
  MergeArgs A;
  A.text1 = r1->d_text; A.qual1 = r1->d_qual; A.text2 = r2->d_text; A.qual2 = r2->d_qual;
  A.start1 = r1->d_table; A.len1 = r1->d_table + n;
  A.start2 = r2->d_table; A.len2 = r2->d_table + n;
  A.bytes1 = r1->text_bytes; A.bytes2 = r2->text_bytes;
  A.rec = s->d_overlaps.p;
  A.table = F->d_table;
  A.n = (uint32_t)n;
  A.n_blocks = (F->text_bytes - 64) / 64;
  A.text = F->d_text; A.qual = F->d_qual; A.rem = F->d_rem;
  const dim3 grid((uint32_t)((A.n_blocks + 1 + 255) / 256)), block(256);
  if (s->profile == PROFILE_IUPAC) hipLaunchKernelGGL(merge_write_kernel<true>, grid, block, 0, st, A);
  else hipLaunchKernelGGL(merge_write_kernel<false>, grid, block, 0, st, A);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));  // (the handle is whole when the call returns, and the records behind A.rec are free again)
  // (the overlap counts its kernel and, as every _reads call, not the Dna look; zero pairs launch nothing and count nothing)
  s->stats.scan_launches += 4;  // the three kernels of the layout scan and the write kernel
  s->stats.candidates = n_merged;  // (sassy_hip_Stats has no field of its own for it)
  return 0;
}

}  // namespace
}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_merge_pairs(sassy_SearcherType* s, const sassy_hip_Reads* r1, const sassy_hip_Reads* r2, uint32_t min_overlap, size_t k,
                          uint32_t max_permille, uint32_t flags, sassy_hip_ReadOverlap* out_overlaps, sassy_hip_Reads** out_merged) {
  if (out_merged) *out_merged = nullptr;
  MrgCall c{};
  c.ovl.have_searcher = s != nullptr;
  c.ovl.have_out = true;  // (the records stay on the device: out_overlaps may be null)
  c.ovl.min_overlap = min_overlap; c.ovl.max_permille = max_permille; c.ovl.flags = flags;
  c.ovl.gate = reads_gate_of(s, 2, r1, r2);
  c.have_merged = out_merged != nullptr;
  // the searcher, the numbers and the pointers first: the batches are read only once nothing else is wrong with the call
  OvlRefusal why_ovl = kOvlOk;
  ReadsRefusal gate = kRdsOk;
  MrgRefusal why = mrg_refusal(c, &why_ovl, &gate);
  if (why != kMrgOverlap) {
    c.ovl.n1 = r1->n_records; c.ovl.n2 = r2->n_records;
    reads_gate_read(s, r1, r2, &c.ovl.gate);
    c.qual1 = r1->d_qual != nullptr; c.qual2 = r2->d_qual != nullptr;
    why = mrg_refusal(c, &why_ovl, &gate);
  }
  if (why == kMrgOverlap) return overlap_refused(why_ovl, gate, c.ovl, "merge_pairs");
  if (why == kMrgNoQuality)
    return fail(SASSY_HIP_EINVAL, std::string("merge_pairs: ") + (c.qual1 ? "r2" : "r1") +
                                      " was parsed without SASSY_HIP_KEEP_QUALITY: a merge needs the base qualities of both batches");
  if (why == kMrgNullMerged) return fail(SASSY_HIP_EINVAL, "Pointers in merge_pairs() must not be null (out_merged)");
  SASSY_NO_TICKETS(s);
  return reads_new_batch(s, kOvlMaxLen, k, out_merged, [&](uint32_t kk, sassy_hip_Reads* F) {  // (k beyond the longest read accepts what k == 512 does)
    return merge_run(s, r1, r2, min_overlap, kk, max_permille, out_overlaps, F);
  });
}

}  // extern "C"
