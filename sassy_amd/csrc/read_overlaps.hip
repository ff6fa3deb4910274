// read_overlaps.hip -- the best overlap of the two reads of a pair (sassy_hip_read_overlaps): pair r is read r
// of R1 against the reverse complement of read r of R2, two read batches resident on the device (fastq_reads.hip).  Every
// offset whose overlap can be accepted is tried; the best accepted one (lowest mismatch density, then the longer overlap,
// then the larger offset) and the number of accepted ones come back, 16 bytes per pair.  The arithmetic -- the refusals, the
// complement, the geometry, the mismatch word, the acceptance, the order -- is overlap_step.h's.
//
// One launch, one wavefront per pair, four pairs per workgroup:
//   planes   64 bytes per step, a lane per byte: the lane's code (for b: of the complement of R2's byte from the far end),
//            one ballot per plane.  a's words stay wave-uniform; b's go to LDS between two zero thirds (overlap_step.h).
//   offsets  the lanes become offsets, 64 per round: a word index and a bit shift per lane, per word and plane two LDS
//            words and one funnel shift, the mismatch word under the range mask, a popcount.  Each lane keeps its best.
//   result   a butterfly over the wavefront with ovl_combine; lane 0 stores the record.
// The handles are only read.  Every load of a read's bytes is bounded by the handle's length table and by its text size.
#include <hip/hip_runtime.h>

#include "host_internal.h"
#include "overlap_step.h"

static_assert(sizeof(sassy_hip_ReadOverlap) == 16, "one 16-byte store per pair");
static_assert(SASSY_HIP_OVERLAP_MAX_LEN == sassy_hip::kOvlMaxLen, "the header's limit is the step header's");

namespace sassy_hip {
namespace {

struct OverlapArgs {
  const uint8_t *text1, *text2;
  const uint64_t *start1, *len1, *start2, *len2;  // the handles' tables
  uint64_t bytes1, bytes2;                        // the handles' text sizes
  uint64_t n;
  uint32_t min_overlap, k, max_permille;
  sassy_hip_ReadOverlap* out;
};

template <int W, bool IUPAC>
__global__ __launch_bounds__(256) void read_overlaps_kernel(OverlapArgs A) {
  constexpr int P = IUPAC ? 4 : 2;
  constexpr uint32_t profile = IUPAC ? kHamIupac : kHamDna;
  // a's words are wave-uniform: they stay in scalar registers where those hold them all, else they go to LDS beside b's
  constexpr bool A_IN_LDS = (P + 1) * W > 48;
  __shared__ uint32_t lds_b[kOvlPairsPerGroup][(P + 1) * 3 * W];
  __shared__ uint32_t lds_a[kOvlPairsPerGroup][A_IN_LDS ? (P + 1) * W : 1];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t pair = (uint64_t)blockIdx.x * kOvlPairsPerGroup + wave;
  const bool live = pair < A.n;
  uint32_t* bpad = lds_b[wave];

  uint64_t s1 = 0, s2 = 0;
  uint32_t la = 0, lb = 0;
  if (live) {
    s1 = A.start1[pair]; s2 = A.start2[pair];
    const uint64_t l1 = A.len1[pair], l2 = A.len2[pair];
    // (the host refused longer reads; a pair that does not fit the instance or its text is left without an overlap)
    const bool fits = l1 <= 32u * W && l2 <= 32u * W && s1 <= A.bytes1 && l1 <= A.bytes1 - s1 && s2 <= A.bytes2 && l2 <= A.bytes2 - s2;
    la = fits ? (uint32_t)l1 : 0u;
    lb = fits ? (uint32_t)l2 : 0u;
  }

  // ---- planes ----
  for (uint32_t i = lane; i < (uint32_t)(P + 1) * 2u * W; i += 64u) {  // the outer thirds
    const uint32_t p = i / (2u * W), j = i % (2u * W);
    bpad[p * 3u * W + (j < (uint32_t)W ? j : j + W)] = 0u;
  }
  uint32_t a_planes[A_IN_LDS ? 1 : (P + 1) * W];
#pragma unroll
  for (int c = 0; c < W / 2; ++c) {
    const uint32_t t = 64u * c + lane;
    const bool in_a = t < la, in_b = t < lb;
    const uint32_t ca = in_a ? ovl_row_code(profile, A.text1[s1 + t], 0) : 0u;
    const uint32_t cb = in_b ? ovl_row_code(profile, A.text2[s2 + (lb - 1u - t)], 1) : 0u;
#pragma unroll
    for (int p = 0; p <= P; ++p) {
      const unsigned long long wa = __ballot(p == P ? in_a : ((ca >> p) & 1u) != 0u);
      const unsigned long long wb = __ballot(p == P ? in_b : ((cb >> p) & 1u) != 0u);
      if constexpr (A_IN_LDS) {
        if (lane < 2u) lds_a[wave][p * W + 2 * c + lane] = lane ? (uint32_t)(wa >> 32) : (uint32_t)wa;
      } else {
        a_planes[p * W + 2 * c] = (uint32_t)wa;
        a_planes[p * W + 2 * c + 1] = (uint32_t)(wa >> 32);
      }
      if (lane < 2u) bpad[p * 3 * W + W + 2 * c + lane] = lane ? (uint32_t)(wb >> 32) : (uint32_t)wb;
    }
  }
  __syncthreads();  // (every wavefront of the workgroup comes here, with or without a pair)

  // ---- offsets ----
  const OvlRange range = ovl_offsets(la, lb, A.min_overlap);
  const int32_t d_last = range.d_first + (int32_t)range.count - 1;
  OvlBest best = ovl_none();
  for (uint32_t round = 0; round < ovl_rounds(range.count); ++round) {
    const int32_t d_mine = range.d_first + (int32_t)(round * kOvlWave + lane);
    const bool in_range = d_mine <= d_last;
    const int32_t d = in_range ? d_mine : d_last;  // (a lane past the last offset repeats it and counts nothing)
    const uint32_t q = ovl_shift_word(W, d), r = ovl_shift_bits(d);
    uint32_t mm = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      uint32_t aw[P + 1], bw[P + 1];
#pragma unroll
      for (int p = 0; p <= P; ++p) {
        aw[p] = A_IN_LDS ? lds_a[wave][p * W + w] : a_planes[p * W + w];
        bw[p] = ovl_shifted_word(bpad, W, p, q, r, w);
      }
      mm = pairs_popcount(ovl_mismatch_word<P, IUPAC>(aw, bw), mm);
    }
    const uint32_t ov = ovl_overlap(la, lb, d);
    best = ovl_combine(best, ovl_one(d, ov, mm, in_range && ovl_accepts(mm, ov, A.min_overlap, A.k, A.max_permille)));
  }

  // ---- the wavefront's result ----
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) {
    OvlBest other;
    other.d = __shfl_xor(best.d, step, 64);
    other.ov = __shfl_xor(best.ov, step, 64);
    other.mm = __shfl_xor(best.mm, step, 64);
    other.n = __shfl_xor(best.n, step, 64);
    best = ovl_combine(best, other);
  }
  if (live && lane == 0u) {
    sassy_hip_ReadOverlap rec;
    rec.offset = best.d; rec.overlap = best.ov; rec.mismatches = best.mm; rec.n_accepted = best.n;
    A.out[pair] = rec;
  }
}

template <bool IUPAC>
hipError_t launch_words(uint32_t W, const OverlapArgs& A, hipStream_t st) {
  const dim3 grid((uint32_t)((A.n + kOvlPairsPerGroup - 1) / kOvlPairsPerGroup)), block(64 * kOvlPairsPerGroup);
  switch (W) {  // ovl_words: reads of at most 64, 128, 192, 256, 512 bytes
    case 2: hipLaunchKernelGGL((read_overlaps_kernel<2, IUPAC>), grid, block, 0, st, A); break;
    case 4: hipLaunchKernelGGL((read_overlaps_kernel<4, IUPAC>), grid, block, 0, st, A); break;
    case 6: hipLaunchKernelGGL((read_overlaps_kernel<6, IUPAC>), grid, block, 0, st, A); break;
    case 8: hipLaunchKernelGGL((read_overlaps_kernel<8, IUPAC>), grid, block, 0, st, A); break;
    default: hipLaunchKernelGGL((read_overlaps_kernel<16, IUPAC>), grid, block, 0, st, A); break;
  }
  return hipGetLastError();
}

// what a refusal of the call's own checks says in a call named `who`
std::string refusal_text(OvlRefusal why, const OvlCall& c, const std::string& w) {
  if (why == kOvlNullSearcher || why == kOvlNullOut) return "Pointers in " + w + "() must not be null";
  if (why == kOvlFlags) return w + " takes no flags (both read batches are on the device)";
  if (why == kOvlMinOverlap) return w + ": min_overlap must be at least 1";
  if (why == kOvlPermille) return w + ": max_permille must be <= 1000 (got " + std::to_string(c.max_permille) + ")";
  if (why == kOvlCounts) return w + ": r1 holds " + std::to_string(c.n1) + " reads, r2 holds " + std::to_string(c.n2) + " (pair r is read r of both)";
  return w + ": refused";
}

// The call behind its refusals.  Timing level >= 1: ev_line[0] -> [1] around the kernel (stats.scan_ms).  out == nullptr (the
// merge): the records stay on the device and, without timing, the stream is not waited for.
int overlaps_run(sassy_SearcherType* s, const sassy_hip_Reads* r1, const sassy_hip_Reads* r2, uint32_t min_overlap, uint32_t k, uint32_t max_permille,
                 sassy_hip_ReadOverlap* out) {
  hipStream_t st = s->stream;
  const uint64_t n = r1->n_records;
  for (const sassy_hip_Reads* r : {r1, r2})  // (as every _reads call, the look is not counted in scan_launches)
    if (int rc = reads_require_plain(s, r, "read_overlaps", r == r1 ? "r1 holds" : "r2 holds", "complement", nullptr)) return rc;
  if ((n + kOvlPairsPerGroup - 1) / kOvlPairsPerGroup > 0x7FFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "read_overlaps: too many pairs for a grid");
  if (int rc = s->d_overlaps.reserve(n)) return rc;
  OverlapArgs A;
  A.text1 = r1->d_text; A.text2 = r2->d_text;
  A.start1 = r1->d_table; A.len1 = r1->d_table + n;
  A.start2 = r2->d_table; A.len2 = r2->d_table + n;
  A.bytes1 = r1->text_bytes; A.bytes2 = r2->text_bytes;
  A.n = n;
  A.min_overlap = min_overlap; A.k = k; A.max_permille = max_permille;
  A.out = s->d_overlaps.p;
  const uint32_t W = ovl_words((uint32_t)std::max(r1->longest, r2->longest));
  if (s->timing >= 1) HIP_TRY(hipEventRecord(s->ev_line[0], st));
  HIP_TRY(s->profile == PROFILE_IUPAC ? launch_words<true>(W, A, st) : launch_words<false>(W, A, st));
  if (s->timing >= 1) HIP_TRY(hipEventRecord(s->ev_line[1], st));
  if (out)
    if (int rc = s->lanes[0].download(out, s->d_overlaps.p, n * sizeof(sassy_hip_ReadOverlap))) return rc;
  if (out || s->timing >= 1) HIP_TRY(hipStreamSynchronize(st));
  if (s->timing >= 1) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, s->ev_line[0], s->ev_line[1]);
    s->stats.scan_ms = ms;
  }
  s->stats.scan_launches = 1;
  s->stats.blocks = (n + kOvlPairsPerGroup - 1) / kOvlPairsPerGroup;
  s->stats.word_rows = W;
  s->stats.text_bytes = (r1->text_bytes - 64) + (r2->text_bytes - 64);
  return 0;
}

}  // namespace

int overlap_refused(uint32_t why, ReadsRefusal gate, const OvlCall& c, const char* who) {
  if (why == kOvlGate)
    return reads_refused(gate, c.gate, ReadsWho{who, "the ascii alphabets have no complement", "scores whole overlaps", "reports the best offset of every pair"});
  return fail(SASSY_HIP_EINVAL, refusal_text((OvlRefusal)why, c, who));
}

int overlaps_resident(sassy_SearcherType* s, const sassy_hip_Reads* r1, const sassy_hip_Reads* r2, uint32_t min_overlap, uint32_t k,
                      uint32_t max_permille, sassy_hip_ReadOverlap* out) {
  return overlaps_run(s, r1, r2, min_overlap, k, max_permille, out);
}

}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_read_overlaps(sassy_SearcherType* s, const sassy_hip_Reads* r1, const sassy_hip_Reads* r2, uint32_t min_overlap, size_t k,
                            uint32_t max_permille, uint32_t flags, sassy_hip_ReadOverlap* out) {
  OvlCall c{};
  c.have_searcher = s != nullptr; c.have_out = out != nullptr;
  c.min_overlap = min_overlap; c.max_permille = max_permille; c.flags = flags;
  c.gate = reads_gate_of(s, 2, r1, r2);
  // the searcher, the numbers and the pointers first: the batches are read only once nothing else is wrong with the call
  ReadsRefusal gate = kRdsOk;
  OvlRefusal why = ovl_refusal(c, &gate);
  if (why == kOvlOk) {
    c.n1 = r1->n_records; c.n2 = r2->n_records;
    reads_gate_read(s, r1, r2, &c.gate);
    why = ovl_refusal(c, &gate);
  }
  if (why != kOvlOk) return overlap_refused(why, gate, c, "read_overlaps");
  SASSY_NO_TICKETS(s);
  if (r1->n_records == 0) return 0;
  const size_t lens[1] = {kOvlMaxLen};
  return hamming_call(s, lens, 1, k, [&](uint32_t kk) {  // (k beyond the longest read accepts what k == 512 does)
    return overlaps_run(s, r1, r2, min_overlap, kk, max_permille, out);
  });
}

}  // extern "C"
