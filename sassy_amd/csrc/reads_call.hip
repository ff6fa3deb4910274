// reads_call.hip -- what surrounds the refusal predicate of every call on a device-resident read batch (read_overlaps,
// merge_pairs, trim_reads, demux_reads, umi_groups_reads, dedup_reads), once: the gate's snapshot of the
// searcher and of the handles, what a refusal of the gate says and returns, the Dna look, and the window call behind
// sassy_hip_reads_slice and sassy_hip_reads_select.  The predicates are reads_gate.h's; the frame of a call that returns a new
// batch is host_internal.h's reads_new_batch.  No kernel lives here.
#include <hip/hip_runtime.h>

#include "host_internal.h"

namespace sassy_hip {

ReadsGate reads_gate_of(const sassy_SearcherType* s, uint32_t handles, const sassy_hip_Reads* r1, const sassy_hip_Reads* r2) {
  ReadsGate g{};
  g.handles = handles;
  g.have_reads[0] = r1 != nullptr; g.have_reads[1] = r2 != nullptr;
  if (s) {
    g.profile = s->profile == PROFILE_DNA ? kHamDna : s->profile == PROFILE_IUPAC ? kHamIupac : 0u;
    g.overhang = !std::isnan(s->alpha) || s->max_overhang >= 0;
    g.only_best = s->only_best;
    g.max_n_frac = !std::isnan(s->max_n_frac);
    g.in_flight = tickets_open(s);
  }
  return g;
}

void reads_gate_read(sassy_SearcherType* s, const sassy_hip_Reads* r1, const sassy_hip_Reads* r2, ReadsGate* g) {
  DeviceGuard on_device(s);  // (first use binds the searcher to the thread's device)
  g->device_s = s->device;
  g->device_r[0] = r1->device; g->longest[0] = r1->longest;
  if (g->handles > 1) { g->device_r[1] = r2->device; g->longest[1] = r2->longest; }
  g->handle_read = true;
}

int reads_refused(ReadsRefusal why, const ReadsGate& g, const ReadsWho& who) {
  const std::string w = who.name;
  const bool pair = g.handles > 1;
  const int code = why == kRdsOverhang || why == kRdsOnlyBest || why == kRdsNFrac ? SASSY_HIP_EUNSUPPORTED : SASSY_HIP_EINVAL;  // (as the family does)
  if (why == kRdsAscii) return fail(code, w + ": " + who.ascii + "; use a dna or an iupac searcher");
  if (why == kRdsOverhang) return fail(code, "the Hamming search does not take overhang (alpha): " + w + " " + who.overhang);
  if (why == kRdsOnlyBest) return fail(code, w + " " + who.only_best + ": only_best_match is not supported");
  if (why == kRdsNFrac) return fail(code, w + " does not take max_n_frac: there is no text span for it to apply to");
  if (why == kRdsNullReads) return fail(code, "Pointers in " + w + "() must not be null");
  if (why == kRdsDevice)
    return fail(code, w + ": the reads were made on device" + (pair ? "s " + std::to_string(g.device_r[0]) + " and " + std::to_string(g.device_r[1])
                                                                     : " " + std::to_string(g.device_r[0])) +
                          ", the searcher is on device " + std::to_string(g.device_s));
  if (why == kRdsTooLong)
    return fail(code, w + " takes reads of at most " + std::to_string(kReadsMaxLen) + " bytes (SASSY_HIP_OVERLAP_MAX_LEN; the longest " +
                          (pair ? "are " + std::to_string(g.longest[0]) + " and " + std::to_string(g.longest[1]) : "has " + std::to_string(g.longest[0])) + ")");
  if (why == kRdsInFlight) return fail(code, "searches are in flight on this searcher (sassy_hip_search_shard_begin): finish them first");
  return fail(code, w + ": refused");
}

int reads_require_plain(sassy_SearcherType* s, const sassy_hip_Reads* reads, const char* who, const char* subject, const char* verb, uint32_t* launches) {
  if (s->profile != PROFILE_DNA) return 0;  // the 2-bit codes and the complement are exact on A, C, G, T only
  TextSource src;
  src.reads = reads;
  bool plain = false;
  if (int rc = reads_plain(s, src, &plain)) return rc;
  if (launches && reads->text_bytes > 64) ++*launches;  // (reads_plain launches over the layout's blocks)
  if (!plain)
    return fail(SASSY_HIP_EINVAL, std::string(who) + ": " + subject + " other bytes than A, C, G, T, which a dna searcher cannot " + verb + ": use an iupac searcher");
  return 0;
}

namespace {

// F: a fresh handle; it is the caller's to release where this fails.
int windows_run(const sassy_hip_Reads* reads, const uint64_t* src, const uint64_t* begins, const uint64_t* lens, uint64_t n_out, hipStream_t st,
                const std::string& who, sassy_hip_Reads* F) {
  const bool keep_quality = reads->d_qual != nullptr;
  F->device = reads->device;
  if (n_out == 0) {
    if (int rc = reads_empty_buffers(F, keep_quality, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  std::vector<uint64_t> whole;
  if (!lens) {  // whole reads: their lengths from the handle's own table
    whole.resize(n_out);
    for (uint64_t j = 0; j < n_out; ++j) whole[j] = reads->records[src ? src[j] : j].seq_len;
    lens = whole.data();
  }
  const uint64_t parts = 1 + (src ? 1 : 0) + (begins ? 1 : 0);
  uint64_t* d_win = nullptr;  // lens[n_out], then begins[n_out] and src[n_out] where given
  if (hipMalloc(reinterpret_cast<void**>(&d_win), parts * n_out * sizeof(uint64_t)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(SASSY_HIP_ENOMEM, who + ": out of device memory (" + std::to_string(parts * n_out * sizeof(uint64_t)) + " bytes of windows)");
  }
  uint64_t *d_begin = begins ? d_win + n_out : nullptr, *d_src = src ? d_win + (parts - 1) * n_out : nullptr;
  int rc = 0;
  hipError_t e = hipMemcpyAsync(d_win, lens, n_out * sizeof(uint64_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && begins) e = hipMemcpyAsync(d_begin, begins, n_out * sizeof(uint64_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && src) e = hipMemcpyAsync(d_src, src, n_out * sizeof(uint64_t), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (windows)");
  if (rc == 0) rc = reads_layout_windows(d_win, n_out, keep_quality, st, F);  // (waits: `whole` has landed)
  if (rc == 0) rc = write_windows(reads, d_src, d_begin, F, st);
  const hipError_t done = hipStreamSynchronize(st);
  (void)hipFree(d_win);
  if (rc == 0 && done != hipSuccess) rc = hip_fail(done, ("hipStreamSynchronize (" + who + ")").c_str());
  return rc;
}

}  // namespace

int windows_from_host(const sassy_hip_Reads* reads, const uint64_t* src, const uint64_t* begins, const uint64_t* lens, uint64_t n_out, hipStream_t st,
                      const char* who, sassy_hip_Reads** out) {
  int cur = 0, prev = -1;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != reads->device) {  // the handle's device, for the length of the call
    HIP_TRY(hipSetDevice(reads->device));
    prev = cur;
  }
  std::unique_ptr<sassy_hip_Reads> F(new sassy_hip_Reads);
  const int rc = windows_run(reads, src, begins, lens, n_out, st, who, F.get());
  if (rc != 0) F->release();
  if (prev >= 0) (void)hipSetDevice(prev);
  if (rc != 0) return rc;
  *out = F.release();
  return 0;
}

}  // namespace sassy_hip
