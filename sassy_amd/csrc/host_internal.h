// host_internal.h -- what the host units of libsassy_hip.so share: the searcher, its lanes and buffers, one scan job,
// the scan queue, the result types, and the functions one unit calls in another.  Units:
//   scan_driver.hip   one pattern over one buffer: ScanJob (prepare / enqueue / finish), strands, search_text
//   many_patterns.hip search_encoded / search_many: pattern-tiled scan, seeded search, lists -> reports -> records
//   multi_device.hip  sassy_hip_multi_*: one text over several devices inside one process
//   hamming.hip       sassy_hip_search_hamming, _search_hamming_many, _hamming_best_pattern, _hamming_counts(_many): the Hamming scan and emit kernels,
//                     the device side of their one driver (ham_prepare, ham_scan_range; records / cells / counts) and the entry points
//   hamming_plan.h    that driver's decisions that need no device (patterns as scanned, groups, tables, overflow step, text batches), free of HIP
//   amplicons.hip     sassy_hip_hamming_amplicons: primer pairs joined on the sorted items of the Hamming scan (ham_walk_ranges, below)
//   fastq_reads.hip   sassy_hip_fastq_parse: FASTQ into a resident read batch; sassy_hip_*_reads, the Hamming batch calls over it
//   read_overlaps.hip sassy_hip_read_overlaps: the best overlap of read r of one resident batch with the reverse complement of read r of another
//   merge_pairs.hip   sassy_hip_merge_pairs: every pair with an accepted overlap merged into a new resident batch, consensus sequence and quality
//   c_abi.hip         the C-ABI of include/sassy.h + sassy_hip.h, the switch table, synthetic inputs
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <iterator>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sassy_hip.h"
#include "common.h"
#include "profiles.h"
#include "switches.h"
#include "pass_planner.h"
#include "scan_route.h"
#include "hamming_plan.h"
#include "reads_gate.h"

namespace sassy_hip {
// (thread_local LaunchEvents g_launch_events: defined in scan_driver.hip, declared in common.h)


// kernel launchers (scan_kernel.hip is compiled once per profile; aux_kernels.hip)
hipError_t launch_scan_dna(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_scan_iupac(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_scan_ascii(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_scan_ascii_ci(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_scan_classes(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);  // (PROFILE_CLASSES)
hipError_t launch_filter_dna(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_filter_group(const ScanParams& P, uint32_t grid, hipStream_t stream);  // (two searches, one pass)
// (one or two searches on kept code planes: src = kPlaneWrite / kPlaneRead)
hipError_t launch_filter_kept(const ScanParams& P, uint32_t grid, uint32_t members, uint32_t src, hipStream_t stream);
hipError_t launch_filter_table(const ScanParams& P, uint32_t grid, hipStream_t stream);
hipError_t launch_filter_dna_multi(const ScanParams& P, uint32_t grid, hipStream_t stream);
hipError_t launch_filter_count(const ScanParams& P, uint32_t grid, hipStream_t stream);
hipError_t launch_count_n(const uint8_t* d_text, const uint64_t* d_range, uint32_t n, uint32_t* d_count,
                          hipStream_t stream);
hipError_t launch_acgt_check(const uint8_t* d_text, uint64_t n, uint32_t* d_flag, hipStream_t stream, int allow_x = 0);
hipError_t launch_reverse_texts(const uint8_t* d_src, uint8_t* d_dst, uint64_t n, const uint32_t* d_blk2text,
                                const uint64_t* d_start, const uint64_t* d_len, uint32_t pad, hipStream_t stream);
hipError_t launch_filter_iupac(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_filter_ascii(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_filter_ascii_ci(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_list_dna(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_list_iupac(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_list_ascii(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_list_ascii_ci(const ScanParams& P, uint32_t grid, size_t smem, hipStream_t stream);
hipError_t launch_build_chunks(const unsigned long long* d_hit, uint64_t n_words, uint64_t n_blocks,
                               uint64_t first_owned, uint32_t wb, uint32_t L, uint32_t maxlen,
                               ChunkDesc* d_desc, uint32_t* d_desc_count, uint32_t desc_cap,
                               unsigned long long* d_hit_count, hipStream_t stream);
hipError_t launch_compact_chunks(const ChunkDesc* d_regions, const uint32_t* d_region_count, uint32_t n_regions, ChunkDesc* d_desc,
                                 uint32_t* d_desc_count, uint32_t desc_cap, uint32_t* d_fuse_word, hipStream_t stream);
hipError_t launch_generate_dna(uint8_t* d_text, uint64_t n, uint64_t seed, uint64_t first, hipStream_t stream);
hipError_t launch_generate_genome_like(uint8_t* d_text, uint64_t n, uint64_t seed, uint64_t first, int with_n,
                                       hipStream_t stream);
hipError_t launch_scatter_bytes(uint8_t* d_text, uint64_t n, uint64_t first, const uint64_t* d_pos,
                                const uint8_t* d_val, uint64_t count, hipStream_t stream);
hipError_t launch_reverse(const uint8_t* d_in, uint8_t* d_out, uint64_t n, hipStream_t stream);
hipError_t launch_trace(const TraceParams& P, uint32_t nblocks, hipStream_t stream);
hipError_t launch_rank(const Candidate* d_cand, const uint32_t* d_count, uint32_t cap, uint32_t* d_rank,
                       Candidate* d_sorted, Candidate* h_sorted, uint32_t host_cap, void* h_ctl,
                       const TextTable& texts, hipStream_t stream);

size_t sort_scratch_bytes(uint32_t count);
hipError_t launch_sort_candidates(const Candidate* d_cand, Candidate* d_sorted, uint32_t count, void* d_scratch,
                                  size_t scratch_bytes, hipStream_t stream, int by_tag = 0, int key_bits = 64);
hipError_t launch_report_flags(const Candidate* d_list, uint32_t max_count, const uint32_t* d_count, uint64_t min_pos,
                               uint32_t* d_flags, hipStream_t stream);
size_t unique_scratch_bytes(uint32_t count);
hipError_t launch_unique_reports(Candidate* d_sorted, uint32_t count, uint64_t min_pos, Candidate* d_out, uint32_t* d_out_count,
                                 void* d_scratch, size_t scratch_bytes, hipStream_t stream);
size_t select_scratch_bytes(uint32_t count);
hipError_t launch_select_reports(const Candidate* d_sorted, uint32_t count, Candidate* d_sel, uint32_t* d_sel_count,
                                 void* d_scratch, size_t scratch_bytes, hipStream_t stream, int all_minima = 0);
hipError_t launch_seed_search(const SeedParams& P, uint32_t grid, hipStream_t stream);
hipError_t launch_pack_text(const uint8_t* d_text, uint64_t n, uint32_t* d_packed, hipStream_t stream);
hipError_t launch_dirty_scan(const uint8_t* d_text, uint64_t n, unsigned long long* d_starts, unsigned long long* d_ends,
                             unsigned long long* d_hard, uint32_t cap, uint32_t* d_counts, hipStream_t stream);
hipError_t launch_gather_zones(const uint8_t* d_text, uint8_t* d_dst, const unsigned long long* d_seg, uint32_t n_seg,
                               hipStream_t stream);
hipError_t launch_map_zone_list(const Candidate* d_in, uint32_t count, const unsigned long long* d_zone, uint32_t n_zones,
                                Candidate* d_out, uint32_t* d_out_count, uint32_t out_cap, hipStream_t stream);
hipError_t launch_drop_excluded(const Candidate* d_in, uint32_t count, const unsigned long long* d_excl, uint32_t n_excl,
                                unsigned char* d_keep, hipStream_t stream);
hipError_t launch_compact_candidates(const Candidate* d_in, uint32_t count, const unsigned char* d_keep, Candidate* d_out,
                                     uint32_t* d_out_count, void* d_scratch, size_t scratch_bytes, hipStream_t stream);
hipError_t launch_tiled_scan(const TiledParams& P, hipStream_t stream);
hipError_t launch_tiled_pertext(const TiledParams& P, hipStream_t stream);
size_t many_scratch_bytes(uint32_t count);
hipError_t launch_assemble_many(const ManyPart& a, const ManyPart& b, uint32_t n_texts, const uint64_t* d_text_len,
                                uint64_t first_text, uint32_t str_stride, MatchOut* d_rows, char* d_strs, uint32_t* d_flags,
                                void* d_scratch, size_t scratch_bytes, hipStream_t stream, int flip = 1, int text_major = 0);
hipError_t launch_assign_texts(Candidate* d_rep, uint32_t count, const TextTable& texts, uint32_t* d_report_text,
                               hipStream_t stream);
hipError_t launch_keep_interior(const Candidate* d_rec, uint32_t count, const TextTable& texts, uint32_t edge, unsigned char* d_keep,
                                hipStream_t stream);
size_t compact_scratch_bytes(uint32_t max_count, uint32_t str_stride);
hipError_t launch_compact_cigars(MatchOut* d_rows, const char* d_strs, uint32_t max_count, const uint32_t* d_count, uint32_t str_stride,
                                 uint32_t* d_total, void* d_scratch, size_t scratch_bytes, const char** d_out_strs, hipStream_t stream);
size_t encoded_scratch_bytes(uint32_t count);
hipError_t launch_assemble_encoded(const MatchOut* d_rows_in, const char* d_strs_in, uint32_t count, uint64_t n_original, uint32_t str_stride,
                                   int key_bits, MatchOut* d_rows, char* d_strs, uint32_t* d_flags, void* d_scratch, size_t scratch_bytes,
                                   hipStream_t stream);


extern thread_local std::string g_err;  // (defined in c_abi.hip: sassy_hip_last_error reads it)
inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
inline int hip_fail(hipError_t e, const char* what) {
  return fail(SASSY_HIP_ENODEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);   \
  } while (0)

// A growable device buffer.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  int reserve(size_t n) {
    if (n <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + n / 8 + 64;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    cap = want;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// sassy_hip_min_costs / _best_pattern in progress (min_costs.hip): where the one-pass batch paths of search_many reduce
// their (pattern, position, cost) list instead of sorting, reporting and tracing it.  The batch functions fill in the
// batch's geometry and arm the sink per batch and strand; an unarmed sink leaves the path as search_many runs it.
struct MinSink {
  uint32_t* d_cells = nullptr;  // device: per pair [pattern * n_cols + text], per text [text]; 0xFFFFFFFF = no match
  bool per_text = false;        // cells hold cost << 25 | pattern << 1 | strand (else cost << 1 | strand)
  uint64_t n_cols = 0;          // texts of the whole call
  uint64_t n_cells = 0;         // cells of the whole call
  bool armed = false;           // this batch's lists are reduced here
  uint64_t col0 = 0;            // the batch's first text
  uint32_t nt = 0;              // texts in the batch
  bool flip = false;            // the Rc strand saw the batch reversed as a whole: its text r is text nt - 1 - r
  uint32_t strand = 0;
  bool used = false;            // some list was reduced into the cells
  // sassy_hip_best_matches (best_matches.hip): one 64-bit cell per text that keeps the winning end position too; when both
  // strands of the batch are reduced, the batch function traces one candidate per cell (finish_best_matches)
  unsigned long long* d_located = nullptr;  // device: [text]; all ones = no match.  != nullptr: this is the call
  bool without_trace = false;   // end and cost only: the records are made from the cells by the host
  bool located = false;         // the result holds the best matches, one record per text that has one
};
hipError_t launch_locate_reduce(const Candidate* d_list, uint32_t count, const TextTable& texts, const MinSink& sink, hipStream_t stream);
// every non-empty cell of texts [col0, col0 + nt) -> the candidate the traceback tail takes, per strand: cand[strand][i] /
// rtext[strand][i] (the text's index in that strand's table), i < d_count[strand] (zeroed by the caller)
hipError_t launch_best_candidates(const unsigned long long* d_cells, uint32_t nt, const TextTable& fwd, const TextTable& rcs, uint32_t flip,
                                  Candidate* d_cand, uint32_t* d_rtext, uint32_t* d_count, hipStream_t stream);
// a cell's fields (the key's layout: best_matches.hip)
constexpr unsigned long long kNoLocated = ~0ull;
inline uint32_t located_cost(unsigned long long c) { return (uint32_t)(c >> 56); }
inline uint32_t located_pattern(unsigned long long c) { return (uint32_t)(c >> 32) & 0xFFFFFFu; }
inline uint32_t located_strand(unsigned long long c) { return (uint32_t)(c >> 31) & 1u; }
inline uint64_t located_end(unsigned long long c) { return 0x7FFFFFFFull - (c & 0x7FFFFFFFull); }
hipError_t launch_min_reduce(const Candidate* d_list, uint32_t count, const TextTable& texts, const MinSink& sink, hipStream_t stream);

}  // namespace sassy_hip

using namespace sassy_hip;

// Pinned, device-mapped host blocks: the kernels write a search's control block, reports, match rows and cigar
// strings straight into one (ScanLane::h_pin).  A result that needs no host-side editing ADOPTS the block instead of
// copying 0.5 MB out of it (17 us of a 0.64 ms search); the lane takes another block from this pool, and
// sassy_hip_result_free puts the adopted one back.
struct PinBlock {
  unsigned char* h = nullptr;
  unsigned char* d = nullptr;  // device address of h
  size_t cap = 0;
  int dev = -1;
};
struct PinPool {
  std::mutex mu;
  std::vector<PinBlock> blocks;
  static constexpr size_t kKeep = 12;
  static constexpr size_t kKeepBytes = (size_t)5 << 30;  // idle blocks kept for reuse (dense results hold 100 MB and more each; a
                                                         // guide set's 17 M matches 2.2 GB -- pinning that again costs more than the search)
  // blocks that results hold right now: a caller who keeps every result alive must not pin memory without bound (and
  // pay a hipHostMalloc per search) -- beyond kMaxAdopted outstanding blocks (or kMaxAdoptedBytes) results are copied
  // out as before
  static constexpr int kMaxAdopted = 16;
  static constexpr size_t kMaxAdoptedBytes = (size_t)8 << 30;
  int adopted = 0;
  size_t adopted_bytes = 0;
  bool may_adopt(size_t bytes) {
    std::lock_guard<std::mutex> g(mu);
    if (adopted >= kMaxAdopted || adopted_bytes + bytes > kMaxAdoptedBytes) return false;
    ++adopted;
    adopted_bytes += bytes;
    return true;
  }
  void adopted_back(size_t bytes) {
    std::lock_guard<std::mutex> g(mu);
    if (adopted > 0) --adopted;
    adopted_bytes -= std::min(adopted_bytes, bytes);
  }
  bool take(size_t bytes, int dev, PinBlock& out) {
    std::lock_guard<std::mutex> g(mu);
    for (size_t i = 0; i < blocks.size(); ++i)
      if (blocks[i].dev == dev && blocks[i].cap >= bytes && blocks[i].cap <= 2 * bytes + (1u << 20)) {
        out = blocks[i];
        blocks.erase(blocks.begin() + (long)i);
        return true;
      }
    return false;
  }
  // newest block in, oldest blocks out: after a few dense searches the pool holds their 100 MB blocks, and a
  // following stream of small results must still find its own block sizes kept (dropping the NEW block instead
  // cost every such search a hipHostFree + hipHostMalloc, about 0.9 ms)
  void give(const PinBlock& b) {
    if (!b.h) return;
    std::vector<PinBlock> drop;
    {
      std::lock_guard<std::mutex> g(mu);
      if (b.cap > kKeepBytes) drop.push_back(b);
      else {
        blocks.push_back(b);
        size_t kept = 0;
        for (const PinBlock& x : blocks) kept += x.cap;
        while (blocks.size() > kKeep || kept > kKeepBytes) {
          kept -= blocks.front().cap;
          drop.push_back(blocks.front());
          blocks.erase(blocks.begin());
        }
      }
    }
    for (const PinBlock& x : drop) (void)hipHostFree(x.h);
  }
};
extern PinPool g_pin_pool;  // (defined in scan_driver.hip)

struct sassy_hip_Result {
  std::vector<sassy_hip_Match> matches;
  std::string pool;
  int exit_state = kStateDecTrue;
  int64_t conditional_index = -1;
  // adopted pinned block (pin.h != nullptr): the rows and the cigar pool live in it, the vectors above are empty
  PinBlock pin;
  const sassy_hip_Match* ext_matches = nullptr;
  size_t ext_n = 0;
  const char* ext_pool = nullptr;
  size_t ext_pool_len = 0;
  // SASSY_HIP_LINE_SPANS: one span per record, in record order
  bool has_line_spans = false;
  std::vector<sassy_hip_LineSpan> line_spans;
  size_t size() const { return pin.h ? ext_n : matches.size(); }
  const sassy_hip_Match* data() const { return pin.h ? ext_matches : matches.data(); }
  const char* pool_data() const { return pin.h ? ext_pool : pool.c_str(); }
  size_t pool_size() const { return pin.h ? ext_pool_len : pool.size(); }
  ~sassy_hip_Result() {
    if (pin.h) g_pin_pool.adopted_back(pin.cap);
    g_pin_pool.give(pin);
  }
};

// One search in flight: everything its ScanJob refers to lives here until sassy_hip_search_finish.
struct sassy_hip_Ticket {
  sassy_SearcherType* owner = nullptr;
  int lane = -1;
  sassy_hip::PatternPlan plan;
  std::vector<uint8_t> pat;
  uint64_t total_len = 0;
  bool without_trace = false;
  bool empty_shard = false;
  double t0 = 0;
  std::shared_ptr<void> job;     // the ScanJob (defined below)
  // shared pass (c_abi.hip): the largest member count among the launches that served it; what a launch made for it after
  // its begin returned; the launches' event slots it holds until it is finished
  uint32_t pass_patterns = 1;
  uint32_t plane_launches = 0;  // launches of its pass that read kept code planes (plane_cache.h)
  int launch_rc = 0;
  bool head_done = false;  // ScanJob::enqueue_head ran (a ticket served by range launches)
  std::vector<struct PassSlot*> slots;
};

// One launch of the shared pass (c_abi.hip): the events the dispatch carries (timing level >= 1) and the event the lanes of
// the tickets it serves wait for.  A searcher owns a few; a slot is taken for a launch and given back when the last ticket
// the launch served is finished.
struct PassSlot {
  hipEvent_t ev_start = nullptr, ev_stop = nullptr, ev_done = nullptr;
  int users = 0;
  bool timed = false;
  const void* lane = nullptr;  // the lane whose stream carries the launch
};
constexpr int kPassSlots = 8;  // (four tickets, two launches each)

struct sassy_hip_Encoded {
  Profile profile;
  bool rc;
  size_t plen;
  std::vector<std::vector<uint8_t>> patterns;  // originals, then (if rc) their reverse complements
  size_t n_original;
};

// Everything one scan pipeline (filter -> chunk list -> DP -> rank -> traceback) needs for itself:
// a stream, its timing events, its device work buffers and the pinned, device-mapped host buffer
// its kernels write the results into.  A searcher owns several lanes so that searches in flight
// overlap (the next search's bandwidth-bound filter runs while the previous one's latency-bound
// DP / rank / traceback kernels finish).
constexpr int kMaxLanes = 4;
struct ScanLane {
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr, ev_f = nullptr, ev_filter_done = nullptr;
  hipEvent_t ev_group = nullptr;  // shared pass: this lane's control block and pattern tables are ready for another lane's pass
  DevBuf<uint8_t> d_state, d_scratch, d_str, d_ctl, d_sort, d_scratch2;
  // The control block has a twin: a search clears the OTHER one behind its last kernel (64 bytes, while the host is busy
  // with this search's result), so the next search on this lane starts with its filter instead of a memset launch.
  DevBuf<uint8_t> d_ctl_twin;
  int ctl_cur = 0;                         // 0: d_ctl, 1: d_ctl_twin holds the running search's control block
  bool ctl_clean[2] = {false, false};      // the block's first 64 bytes are zero (cleared behind the previous search)
  hipEvent_t ev_done = nullptr;            // recorded behind a search's last kernel, in front of the twin's clear
  DevBuf<uint32_t> d_flags;     // dense results: "does any record need the host's attention" (report_flags_kernel)
  DevBuf<Candidate> d_cand, d_sorted;
  DevBuf<MatchOut> d_trace;
  DevBuf<ChunkDesc> d_desc, d_regions;   // (d_regions / d_region_count: the counting filter's own chunk list, one region per wave)
  DevBuf<uint32_t> d_region_count;
  DevBuf<uint32_t> d_carry;     // per-row carries of patterns too long for LDS (ScanParams::carry_global)
  // pattern-dependent device data of the scan that runs on this lane, and what it currently holds
  // (uploads are skipped when the pattern repeats); per lane, so that scans of different patterns
  // can be in flight on different lanes
  DevBuf<uint8_t> d_pattern, d_table;
  DevBuf<TextStash> d_stash;   // fused filter: the text under the reports, for the traceback
  DevBuf<unsigned long long> d_probe;  // SASSY_HIP_TRACE_PROBE
  DevBuf<uint32_t> d_rowoff, d_ovtab;
  DevBuf<uint32_t> d_classtab;   // class patterns: the cube table of the scan, the slot bitmaps of the traceback
  DevBuf<uint8_t> d_classbits;
  std::vector<uint8_t> up_pattern, h_table, table_pattern, up_classbits;
  std::vector<uint32_t> up_rowtab, up_ovtab, up_classtab;
  int up_profile = -1, table_profile = -1;
  uint32_t table_q = 0, table_k = 0, table_r = 0;   // table_r: 0 = piece bit table, else the counting table's R
  bool table_rc = false;                            // the counting table also holds the Rc strand's q-grams
  uint32_t fuse_backoff = 0;                        // searches this lane still runs unfused after a fused one overflowed
  double table_density = 0;
  // pinned host staging area: control block and the first kSpec reports of a scan are written into
  // it by the kernels themselves; one stream synchronisation makes them readable
  unsigned char* h_pin = nullptr;
  unsigned char* h_pin_dev = nullptr;  // device address of h_pin
  size_t h_pin_cap = 0;
  bool ready = false;
  // small host -> device uploads (pattern, row table, tables) go through pinned memory: a copy from
  // pageable memory makes the host wait for the device, which serialises the lanes of a ScanQueue
  uint8_t* h_up = nullptr;
  size_t h_up_cap = 0, h_up_used = 0;
  int upload(void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return 0;
    const size_t need = h_up_used + ((bytes + 63) & ~(size_t)63);
    if (need > h_up_cap) {
      if (h_up_used != 0) {  // no room left behind the copies already queued: an ordinary copy
        hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
        return e == hipSuccess ? 0 : hip_fail(e, "hipMemcpyAsync");
      }
      if (h_up) (void)hipHostFree(h_up);
      h_up = nullptr;
      h_up_cap = 0;
      const size_t want = std::max<size_t>(need * 2, 256 * 1024);
      hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&h_up), want, hipHostMallocDefault);
      if (e != hipSuccess) {  // no pinned memory to be had: an ordinary (host-blocking) copy
        (void)hipGetLastError();
        h_up = nullptr;
        e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
        return e == hipSuccess ? 0 : hip_fail(e, "hipMemcpyAsync");
      }
      h_up_cap = want;
    }
    memcpy(h_up + h_up_used, src, bytes);
    hipError_t e = hipMemcpyAsync(dst, h_up + h_up_used, bytes, hipMemcpyHostToDevice, stream);
    h_up_used = need;
    return e == hipSuccess ? 0 : hip_fail(e, "hipMemcpyAsync");
  }
  // Results too large for the device-mapped staging area (dense matches: 10^5 .. 10^6 records) come back with
  // ordinary copies.  A copy into pageable memory runs at ~5 GB/s; through two pinned 8 MiB buffers, the next
  // piece in flight while the previous one is moved to its final place, the transfer runs at the speed of the
  // host memcpy.
  static constexpr size_t kBulk = 8u << 20;
  unsigned char* h_bulk[2] = {nullptr, nullptr};
  int download(void* dst, const void* d_src, size_t bytes) {
    if (bytes == 0) return 0;
    for (unsigned char*& b : h_bulk)
      if (!b && hipHostMalloc(reinterpret_cast<void**>(&b), kBulk, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        b = nullptr;
      }
    if (!h_bulk[0] || !h_bulk[1] || bytes < (1u << 20)) {  // small, or no pinned memory to be had
      hipError_t e = hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      return e == hipSuccess ? 0 : hip_fail(e, "hipMemcpy (results)");
    }
    unsigned char* out = static_cast<unsigned char*>(dst);
    const unsigned char* src = static_cast<const unsigned char*>(d_src);
    size_t issued = 0, done = 0;
    int slot = 0;
    size_t len[2] = {0, 0};
    // prime one piece, then: wait for piece i, issue piece i+1, move piece i
    len[0] = std::min(kBulk, bytes);
    hipError_t e = hipMemcpyAsync(h_bulk[0], src, len[0], hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync (results)");
    issued = len[0];
    while (done < bytes) {
      e = hipStreamSynchronize(stream);
      if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize (results)");
      const int cur = slot;
      slot ^= 1;
      if (issued < bytes) {
        len[slot] = std::min(kBulk, bytes - issued);
        e = hipMemcpyAsync(h_bulk[slot], src + issued, len[slot], hipMemcpyDeviceToHost, stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync (results)");
        issued += len[slot];
      }
      memcpy(out + done, h_bulk[cur], len[cur]);
      done += len[cur];
    }
    return 0;
  }
  int h_pin_device = -1;
  int reserve_pinned(size_t bytes) {
    if (bytes <= h_pin_cap) return 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (h_pin) g_pin_pool.give(PinBlock{h_pin, h_pin_dev, h_pin_cap, h_pin_device});
    h_pin = nullptr;
    h_pin_cap = 0;
    PinBlock b;
    if (g_pin_pool.take(bytes, dev, b)) {
      h_pin = b.h; h_pin_dev = b.d; h_pin_cap = b.cap; h_pin_device = b.dev;
      return 0;
    }
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&h_pin), bytes, hipHostMallocMapped);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc");
    e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h_pin_dev), h_pin, 0);
    if (e != hipSuccess) return hip_fail(e, "hipHostGetDevicePointer");
    h_pin_cap = bytes;
    h_pin_device = dev;
    return 0;
  }
  // hands the block to a result; the next search reserves another one (from the pool)
  PinBlock take_pin() {
    PinBlock b{h_pin, h_pin_dev, h_pin_cap, h_pin_device};
    h_pin = h_pin_dev = nullptr;
    h_pin_cap = 0;
    return b;
  }
  int init() {
    if (ready) return 0;
    if (!stream) {
      HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      own_stream = true;
    }
    HIP_TRY(hipEventCreate(&ev_a));
    HIP_TRY(hipEventCreate(&ev_b));
    HIP_TRY(hipEventCreate(&ev_c));
    HIP_TRY(hipEventCreate(&ev_f));
    HIP_TRY(hipEventCreateWithFlags(&ev_filter_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev_group, hipEventDisableTiming));
    ready = true;
    return 0;
  }
  void destroy() {
    if (h_up) (void)hipHostFree(h_up);
    h_up = nullptr; h_up_cap = h_up_used = 0;
    d_state.release(); d_scratch.release(); d_str.release(); d_ctl.release(); d_ctl_twin.release(); d_sort.release(); d_scratch2.release(); d_flags.release();
    for (unsigned char*& b : h_bulk) { if (b) (void)hipHostFree(b); b = nullptr; }
    d_cand.release(); d_sorted.release(); d_trace.release(); d_desc.release(); d_regions.release(); d_region_count.release(); d_carry.release();
    d_pattern.release(); d_table.release(); d_rowoff.release(); d_ovtab.release(); d_stash.release();
    d_classtab.release(); d_classbits.release();
    if (h_pin) g_pin_pool.give(PinBlock{h_pin, h_pin_dev, h_pin_cap, h_pin_device});
    h_pin = nullptr;
    for (hipEvent_t e : {ev_a, ev_b, ev_c, ev_f, ev_filter_done, ev_done, ev_group})
      if (e) (void)hipEventDestroy(e);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

// The searcher.  Mirrors the configuration surface of the reference's Searcher<P>
// (rc, alpha; reference: src/search.rs:227-256, 486-503) and caches device buffers the way the
// reference caches its host buffers.
// On-line choice of the lane-chunk length of the prefilter for a resident text.  The kernel time depends
// chaotically on it (HBM channel mapping against the lane stride and the lane count: +-10 % between
// neighbouring even values, see stream_geometry), so the first searches of a (text, filter kind) try
// the even values around the default, two calls each, and the rest use the fastest.  Every trial is a
// complete, correct search; only its prefilter geometry differs.
struct GeoTuner {
  const void* text = nullptr;
  uint64_t len = 0, owned = 0;
  uint32_t kind = 0, extra = 0;
  std::vector<uint32_t> cand;
  std::vector<float> best;
  uint32_t trials = 0, chosen = 0;
  // the chunk length to use for this call (0: the default)
  uint32_t next(const void* t, uint64_t l, uint64_t own, uint32_t k, uint32_t ex, uint32_t dflt, uint32_t min_bpl) {
    if (t != text || l != len || own != owned || k != kind || ex != extra) {
      text = t; len = l; owned = own; kind = k; extra = ex;
      cand.clear();
      for (int d = 0; d <= 14; d += 2) {
        for (int sgn = (d ? -1 : 1); sgn <= 1; sgn += 2) {
          const int64_t v = (int64_t)dflt + sgn * d;
          if (v >= (int64_t)min_bpl && v >= 4) cand.push_back((uint32_t)v);
        }
      }
      // ... and around two thirds of it (half again as many lanes: the other basin seen in the sweeps)
      for (int d = -2; d <= 2; d += 2) {
        const int64_t v = ((int64_t)dflt * 2 / 3) / 2 * 2 + d;
        if (v >= (int64_t)min_bpl && v >= 4 && std::find(cand.begin(), cand.end(), (uint32_t)v) == cand.end())
          cand.push_back((uint32_t)v);
      }
      best.assign(cand.size(), 1e30f);
      trials = 0;
      chosen = 0;
    }
    if (chosen) return chosen;
    if (trials < 2 * cand.size()) return cand[trials % cand.size()];
    size_t b = 0;
    for (size_t i = 1; i < cand.size(); ++i)
      if (best[i] < best[b]) b = i;
    chosen = cand[b];
    return chosen;
  }
  void report(uint32_t bpl, float ms) {
    if (chosen) return;
    for (size_t i = 0; i < cand.size(); ++i)
      if (cand[i] == bpl) { best[i] = std::min(best[i], ms); break; }
    ++trials;
  }
};

// A read batch resident on the device (fastq_reads.hip makes it; reads_relayout.hip lays it out anew for search_many).
struct sassy_hip_Reads {
  std::unique_ptr<sassy_hip_ReadRecord[]> records;  // n_records of them, not cleared before the device's copy lands: a
  uint64_t n_records = 0;                           // table of millions of reads is touched once
  uint8_t* d_text = nullptr;
  uint64_t text_bytes = 0;      // the layout and the 64 spare bytes behind it
  uint64_t* d_table = nullptr;  // starts[n], then lens[n]: the order d_ham_texts has
  uint32_t* d_rem = nullptr;    // per block of the layout
  uint8_t* d_qual = nullptr;    // the qualities in the text's layout, text_bytes of them; null where they were not kept
  uint64_t longest = 0;
  int device = -1;
  void release() {
    if (d_text) (void)hipFree(d_text);
    if (d_table) (void)hipFree(d_table);
    if (d_rem) (void)hipFree(d_rem);
    if (d_qual) (void)hipFree(d_qual);
    d_text = nullptr; d_table = nullptr; d_rem = nullptr; d_qual = nullptr;
  }
};

struct sassy_SearcherType {
  // every path-forcing / tuning switch (switches.h): defaults + the environment, read ONCE, here, when the searcher is
  // made; sassy_hip_set_option changes an entry afterwards.  apply_switches() copies the entries that have setters of
  // their own (sassy_hip_set_fused / _reference_lanes / _pipe_depth / _geometry_tuner / _timing) into their members.
  Switches sw = load_switches();
  void apply_switches() {
    fuse = sw.fused != 0;
    ref_lanes = (sw.ref_lanes == 4 || sw.ref_lanes == 8) ? (uint32_t)sw.ref_lanes : 0u;
    pipe_depth = (int)std::max<long>(1, std::min<long>(sw.pipe_depth, kMaxLanes));
    tune = sw.tune != 0;
    timing = (int)sw.timing;
  }
  sassy_SearcherType() { apply_switches(); }
  Profile profile = PROFILE_DNA;
  bool rc = false;
  // lanes[0].stream doubles as the searcher's stream: text / pattern uploads and every search that
  // is not one of several in flight run on it (sassy_hip_set_stream replaces it)
  ScanLane lanes[kMaxLanes];
  hipStream_t stream = nullptr;
  hipStream_t user_stream = nullptr;
  hipEvent_t ev_inputs = nullptr;  // "uploads of this call are queued" (other lanes wait for it)
  bool device_ready = false;
  // The HIP device all of this searcher's streams, buffers and launches live on: the calling thread's current device at
  // the searcher's first search (HIP's current device is per host thread), or sassy_hip_set_device before it.  Every
  // entry point switches to it for the duration of the call (DeviceGuard), whatever thread it is called from.
  int device = -1;
  bool bound = false;  // an entry point has run on `device` (streams / buffers / events may exist there): it stays
  DevBuf<uint8_t> d_text, d_rev;
  DevBuf<unsigned long long> d_rc_bitmap;  // the Rc strand's candidate blocks, marked by the forward pass
  // search_many lays its texts out in pinned host memory (no zero fill, H2D at the PCIe rate, reused
  // across calls)
  uint8_t* h_stage = nullptr;
  size_t h_stage_cap = 0;
  bool h_stage_pinned = false;
  void free_stage() {
    if (h_stage) {
      if (h_stage_pinned) (void)hipHostFree(h_stage);
      else free(h_stage);
    }
    h_stage = nullptr;
    h_stage_cap = 0;
  }
  int reserve_stage(size_t bytes) {
    if (bytes <= h_stage_cap) return 0;
    free_stage();
    const size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&h_stage), want, hipHostMallocDefault);
    h_stage_pinned = e == hipSuccess;
    if (!h_stage_pinned) {  // no pinned memory to be had (locked-memory limit): ordinary memory, slower upload
      (void)hipGetLastError();
      h_stage = static_cast<uint8_t*>(malloc(want));
      if (!h_stage) return fail(SASSY_HIP_ENOMEM, "out of host memory (text staging)");
    }
    h_stage_cap = want;
    return 0;
  }
  const uint8_t* rev_src = nullptr;  // d_rev holds reverse(rev_src[0 .. rev_len)) (SASSY_HIP_TEXT_UNCHANGED)
  uint64_t rev_len = 0;

  bool want_counters = false;
  int prefilter = -1;            // sassy_hip_set_prefilter: -1 process default, 0 never, 1 also with short pieces
  // sassy_hip_set_fused / SASSY_HIP_FUSED: the bit-plane filter runs the chunk DP of what it finds itself (one launch
  // instead of filter -> chunk list -> list kernel); 0 = always the classic chain
  bool fuse = true;
  // sassy_hip_set_reference_lanes: 0 = the definition (one pass), 4 / 8 = the reference binary's lane reports
  // (anything but 4 or 8 in the environment is ignored, as the setter rejects it)
  uint32_t ref_lanes = 0;
  // searches in flight (sassy_hip_search_shard_begin / sassy_hip_search_finish): the ticket that owns each lane
  struct sassy_hip_Ticket* lane_ticket[kMaxLanes] = {nullptr, nullptr, nullptr, nullptr};
  int last_begun_lane = -1;
  int pipe_depth = 2;
  // shared pass (switch shared_pass): which ticket still needs which half of its pass (pass_planner.h), the launches' event
  // slots, and the event that marks the end of the searcher's last launched pass
  sassy_hip::PassPlanner planner;
  PassSlot pass_slots[kPassSlots];
  hipEvent_t last_pass_event = nullptr;
  // kept code planes (switch plane_cache; plane_cache.h): what is written and may be read, and the store itself --
  // allocated at the first launch that can use it, reused while the size fits, freed with the searcher
  sassy_hip::PlaneCache planes;
  uint4* plane_store = nullptr;
  uint64_t plane_store_bytes = 0;
  // reporting modes of the reference's Searcher (src/search.rs:442-475)
  float alpha = NAN;             // overhang cost per pattern character (NaN = no overhang), Iupac only
  long max_overhang = -1;        // with_max_overhang(): -1 = none
  bool only_best = false;        // only_best_match(): one match per strand, minimal cost, rightmost end
  float max_n_frac = NAN;        // with_max_n_frac(): NaN = off (the reference's None)
  GeoTuner tuner, tuner_scan;    // prefilter / streaming-DP geometry per resident text
  // the on-line geometry tuner is opt-in (sassy_hip_set_geometry_tuner, SASSY_HIP_TUNE=1): see stream_geometry
  bool tune = false;
  DevBuf<uint64_t> d_tables;     // multi-text buffers: start / len tables (both strands)
  DevBuf<unsigned long long> d_multi_bitmap;  // multi-pattern prefilter: one hit bitmap per pattern of the batch
  DevBuf<uint32_t> d_multi_bits;
  // pattern-tiled search (search_encoded_tiled): match masks, the patterns' bytes, counters, the selected reports
  DevBuf<unsigned long long> d_tiled_peq;
  DevBuf<uint8_t> d_tiled_pat;
  DevBuf<uint32_t> d_tiled_cnt, d_tiled_rtext;
  DevBuf<Candidate> d_tiled_sel, d_tiled_list;  // (the list is not a lane's d_cand: its size must not leak into single searches)
  // best-cost search (min_costs.hip): the 32-bit cells of the device reduction, the narrowed outputs; the call in progress
  DevBuf<uint32_t> d_min_cells;
  DevBuf<uint8_t> d_min_out;
  sassy_hip::MinSink* min_sink = nullptr;
  // best_matches (best_matches.hip): the 64-bit cells; both strands' candidates, their texts and patterns for the traceback
  DevBuf<unsigned long long> d_best_cells;
  DevBuf<Candidate> d_best_cand;
  DevBuf<uint32_t> d_best_rtext;
  DevBuf<uint8_t> d_best_pat;
  // seeded search (search_encoded_seeded): the piece tables; sub-piece table, packed text and patterns
  DevBuf<uint32_t> d_seed_start[2], d_seed_entries[2], d_seed_sub, d_seed_packed, d_seed_bits, d_seed_e16;
  // ... on texts with other letters (seeded_dirty_zones): run lists / tables, the gathered neighbourhoods, their scan
  DevBuf<unsigned long long> d_zone_u64, d_zone_tab, d_zone_peq;
  DevBuf<uint8_t> d_zone_text;
  DevBuf<Candidate> d_zone_list;
  hipEvent_t ev_multi = nullptr, ev_multi_a = nullptr;
  hipEvent_t ev_a_multi() { return ev_multi_a; }
  // line resolution (line_index.hip): tile offsets | super-tile counts, the super-tile prefix, the spans' ends, the spans;
  // the HIP-event times of the last call's index and resolve passes (timing level 2)
  DevBuf<uint32_t> d_line_tiles;
  DevBuf<unsigned long long> d_line_prefix;
  DevBuf<uint64_t> d_line_pos;
  DevBuf<sassy_hip_LineSpan> d_line_out;
  double line_index_ms = 0, line_resolve_ms = 0;
  hipEvent_t ev_line[4] = {nullptr, nullptr, nullptr, nullptr};  // index pass begin / end, resolve pass begin / end
  // Hamming search (hamming.hip): the pattern tables of a launch, the item counter, the items as written and sorted (laid
  // out as candidates for the sort), the sort's scratch, the items' popcount prefix
  DevBuf<uint32_t> d_ham_tab, d_ham_count, d_ham_prefix;
  DevBuf<Candidate> d_ham_items, d_ham_sorted;
  DevBuf<uint8_t> d_ham_sort;
  // ... over a batch of texts: the (start, len) table, rem per block, the best-pattern cells
  DevBuf<uint64_t> d_ham_texts;
  DevBuf<uint32_t> d_ham_rem;
  DevBuf<unsigned long long> d_ham_cells;
  DevBuf<unsigned long long> d_ham_bins;  // hamming_counts: the copies of the counts table
  // amplicons (amplicons.hip): the join's pattern table, the partners per left hit, their exclusive scan, a launch's records
  DevBuf<uint32_t> d_amp_tab, d_amp_counts;
  DevBuf<uint64_t> d_amp_offs;
  DevBuf<sassy_hip_Amplicon> d_amp_out;
  // all-vs-all Hamming (hamming_pairs.hip): the entries' and the target records' bit planes, the partials matrix (one
  // PairsCell per chunk and entry), the row sums | their scan | its block sums, the records or the nearest columns
  DevBuf<uint32_t> d_pairs_a, d_pairs_t;
  DevBuf<uint4> d_pairs_cells;
  DevBuf<unsigned long long> d_pairs_rows;
  DevBuf<uint8_t> d_pairs_out;
  // UMI groups (umi_groups.hip): what is sized by the reads (the table, rep, count, the flags and their scan, the output
  // columns) and what is sized by the distinct sequences (their planes, counts, labels)
  DevBuf<uint8_t> d_umi_reads, d_umi_distinct;
  DevBuf<sassy_hip_ReadOverlap> d_overlaps;  // read overlaps (read_overlaps.hip): one record per pair
  DevBuf<sassy_hip_ReadTrim> d_trims;        // trimming (trim_reads.hip): one record per read, and the adapter table
  DevBuf<uint32_t> d_trim_tab;
  // demultiplexing (demux_reads.hip): the barcode table, and one area for the records, the labels, the order, the windows and
  // the sort's own scratch
  DevBuf<uint32_t> d_demux_tab;
  DevBuf<uint8_t> d_demux;
  // deduplication (dedup_reads.hip): one area for the window flags and their scan, the reads' table, the columns per read, the
  // scores, the groups' best keys, the kept flags and their scan, the kept reads' table and lengths
  DevBuf<uint8_t> d_dedup;
  DevBuf<uint64_t> d_range;     // N counting on device-resident text
  DevBuf<uint32_t> d_ncount;
  // HIP-event timing of the call's phases: 0 none, 1 the dominant kernel only (filter / streaming
  // scan; default), 2 every phase.  Each event record costs a few microseconds of stream idle time.
  int timing = 1;
  sassy_hip_Stats stats{};
  // the drop-in search() over several devices (SASSY_HIP_DEVICES): a multi-device searcher of this searcher's alphabet
  // and strands, made at the first such call (sassy_hip_Multi is defined further down: owned through its deleter)
  std::shared_ptr<void> multi;

  ~sassy_SearcherType() {
    for (ScanLane& l : lanes)  // searches still in flight (tickets never finished): let their kernels drain
      if (l.stream) (void)hipStreamSynchronize(l.stream);
    // (halves that were never launched are dropped with their tickets)
    for (PassSlot& ps : pass_slots)
      for (hipEvent_t e : {ps.ev_start, ps.ev_stop, ps.ev_done})
        if (e) (void)hipEventDestroy(e);
    for (sassy_hip_Ticket*& t : lane_ticket) { delete t; t = nullptr; }
    if (plane_store) (void)hipFree(plane_store);
    d_text.release(); d_rev.release(); d_rc_bitmap.release();
    free_stage();
    d_line_tiles.release(); d_line_prefix.release(); d_line_pos.release(); d_line_out.release();
    d_ham_tab.release(); d_ham_count.release(); d_ham_prefix.release(); d_ham_items.release(); d_ham_sorted.release(); d_ham_sort.release();
    d_ham_texts.release(); d_ham_rem.release(); d_ham_cells.release(); d_ham_bins.release();
    d_pairs_a.release(); d_pairs_t.release(); d_pairs_cells.release(); d_pairs_rows.release(); d_pairs_out.release();
    d_umi_reads.release(); d_umi_distinct.release(); d_overlaps.release(); d_trims.release(); d_trim_tab.release(); d_demux_tab.release(); d_demux.release();
    d_dedup.release();
    d_range.release(); d_ncount.release(); d_tables.release(); d_multi_bitmap.release(); d_multi_bits.release();
    d_tiled_peq.release(); d_tiled_pat.release(); d_tiled_cnt.release(); d_tiled_sel.release(); d_tiled_list.release(); d_tiled_rtext.release();
    d_min_cells.release(); d_min_out.release();
    d_best_cells.release(); d_best_cand.release(); d_best_rtext.release(); d_best_pat.release();
    for (int t = 0; t < 2; ++t) { d_seed_start[t].release(); d_seed_entries[t].release(); }
    d_seed_sub.release(); d_seed_packed.release(); d_seed_bits.release(); d_seed_e16.release();
    d_zone_u64.release(); d_zone_tab.release(); d_zone_peq.release(); d_zone_text.release(); d_zone_list.release();
    if (ev_multi) (void)hipEventDestroy(ev_multi);
    if (ev_multi_a) (void)hipEventDestroy(ev_multi_a);
    for (hipEvent_t e : ev_line)
      if (e) (void)hipEventDestroy(e);
    for (ScanLane& l : lanes) l.destroy();
    if (ev_inputs) (void)hipEventDestroy(ev_inputs);
  }

  int ensure_device() {
    if (device_ready) return 0;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
      return fail(SASSY_HIP_ENODEVICE,
                  "no usable HIP device (libsassy_hip has no CPU fallback; the scan runs on gfx950 only)");
    lanes[0].stream = user_stream;  // null: the lane creates its own
    for (ScanLane& l : lanes) {
      if (int rc = l.init()) return rc;
    }
    stream = lanes[0].stream;
    HIP_TRY(hipEventCreateWithFlags(&ev_inputs, hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&ev_multi));
    HIP_TRY(hipEventCreate(&ev_multi_a));
    for (hipEvent_t& e : ev_line) HIP_TRY(hipEventCreate(&e));
    device_ready = true;
    return 0;
  }
};

namespace sassy_hip {

inline double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}


// ------------------------------------------------------------------ scan driver
struct ShardView {
  const uint8_t* d_text;   // device buffer (halo first)
  uint64_t text_len;       // bytes in the buffer
  uint64_t halo_len;       // bytes before the first owned block
  uint64_t global_offset;  // global position of d_text[0]
  bool text_start;         // buffer byte 0 is column 0 of the whole text
  bool text_end;           // buffer end is the end of the whole text
  bool adopt_ok = false;   // the caller takes the result as it comes (no reporting modes, no strand merge): it may
                           // stay in the pinned block the kernels wrote it into (ScanOut::pin)
};

struct ScanOut {
  std::vector<Candidate> cands;  // sorted by pos, unconditional (COND resolved) ...
  int64_t conditional_index = -1; // ... except this one, which depends on the previous shard
  int exit_state = kStateDecTrue;
  uint64_t cond_seen = 0;
  // device traceback results (empty without trace): one finished record per candidate, in the
  // same order, whose cigar_off points into `pool`
  std::vector<sassy_hip_Match> matches;
  std::string pool;
  // ... or, adopted (pin.h != nullptr; cands / matches / pool above stay empty), in the pinned block itself
  PinBlock pin;
  ScanOut() = default;
  ScanOut(const ScanOut&) = delete;
  ScanOut& operator=(const ScanOut&) = delete;
  ScanOut(ScanOut&& o) noexcept { *this = std::move(o); }
  ScanOut& operator=(ScanOut&& o) noexcept {
    if (this != &o) {
      if (pin.h) g_pin_pool.adopted_back(pin.cap);
      g_pin_pool.give(pin);
      cands = std::move(o.cands); conditional_index = o.conditional_index; exit_state = o.exit_state; cond_seen = o.cond_seen;
      matches = std::move(o.matches); pool = std::move(o.pool);
      pin = o.pin; o.pin = PinBlock{};
      ext_matches = o.ext_matches; ext_n = o.ext_n; ext_pool = o.ext_pool; ext_pool_len = o.ext_pool_len;
    }
    return *this;
  }
  ~ScanOut() {
    if (pin.h) g_pin_pool.adopted_back(pin.cap);
    g_pin_pool.give(pin);
  }
  const sassy_hip_Match* ext_matches = nullptr;
  size_t ext_n = 0;
  const char* ext_pool = nullptr;
  size_t ext_pool_len = 0;
};
static_assert(sizeof(MatchOut) == sizeof(sassy_hip_Match) && sizeof(MatchOut) == 64, "record layout");

inline uint32_t warmup_blocks(uint32_t m, uint32_t k) { return (m + k + 1 + 63) / 64; }

// One report's traceback slice (trace_kernel.hip), from the shape (m, k) alone: the byte sizes of its parts, the slice
// stride of either kernel shape, and what follows from them.  Every host site that fills a TraceParams reads this.
struct TraceShape {
  uint64_t band;           // (m + 1) rows of 2k + 3 cells (two bytes per cell from k = 255 on)
  uint64_t win;            // the text window, whole 16-byte chunks
  uint64_t ops;            // the edit operations, one byte each
  uint64_t str;            // = TraceParams::str_stride: one record's cigar string
  uint64_t raw;            // band + win + ops + str
  uint64_t pat_bytes;      // the pattern next to the slices
  uint64_t wave_stride;    // wave kernel: raw + kTraceWaveDummy (the band rows' lanes outside the band store there, unmasked;
                           // the kernel finds them at scratch_stride - kTraceWaveDummy)
  uint64_t thread_stride;  // thread kernel: raw, bumped to an odd number of LDS words (conflict-free slices)
  bool wave_fits;          // a band row fits a wavefront, and four slices with their patterns fit a CU's LDS
  bool thread_in_lds;      // the thread kernel's 64 slices per workgroup fit LDS (else: global memory)
  uint64_t thread_count;   // slices in LDS: threads of a launch with as many workgroups as the chip holds at once
};
inline TraceShape trace_shape(uint32_t m, uint32_t k) {
  TraceShape s{};
  const uint64_t cell = (k + 1 <= 255) ? 1 : 2;
  s.band = ((uint64_t)(m + 1) * (2ull * k + 3) * cell + 3) / 4 * 4;
  s.win = ((uint64_t)m + k + 15 + 15) / 16 * 16;
  s.ops = ((uint64_t)m + k + 1 + 3) / 4 * 4;
  s.str = (2ull * (m + k + 1) + 2 + 15) / 16 * 16;
  s.raw = s.band + s.win + s.ops + s.str;
  s.pat_bytes = ((uint64_t)m + 15) / 16 * 16;
  s.wave_stride = (s.raw + kTraceWaveDummy + 15) / 16 * 16;
  s.thread_stride = s.raw + ((s.raw / 4) % 2 == 0 ? 4 : 0);
  s.wave_fits = 2ull * k + 3 <= 64 && 4 * s.pat_bytes + 4 * s.wave_stride <= 160 * 1024;
  const uint64_t wg_bytes = 64 * s.thread_stride + s.pat_bytes;
  s.thread_in_lds = wg_bytes <= kTraceLdsLimit;
  s.thread_count = std::min<uint64_t>(256ull * 64ull * std::max<uint64_t>(1, (160ull * 1024) / wg_bytes), 131072);
  return s;
}

// One scan of one buffer (a whole text or a shard) on one lane, in three phases so that several can be
// in flight: prepare() sizes everything and uploads what the pattern needs, enqueue() queues the
// whole kernel pipeline on the lane's stream without waiting, finish() waits for it, grows buffers
// and re-runs on overflow, and turns the device output into resolved reports.
// Two exact paths: the streaming DP over every block, or -- when the pattern splits into k+1
// selective pieces -- prefilter (K0) -> chunk list (K0b) -> DP over the listed chunks (K1-list).
struct ScanJob {
  sassy_SearcherType* S;
  ScanLane& L;
  ShardView sh;
  const PatternPlan& plan;
  uint32_t k;
  bool all_minima;
  const uint8_t* pat;
  bool do_trace;
  uint64_t total_len;
  TextTable texts{};                 // several texts in the buffer (n = 0: one text)
  // multi-pattern search: the hit bitmap was filled by filter_dna_multi_kernel (piece length ext_q);
  // this job only waits for it (ext_wait) and runs chunk list -> DP -> rank -> traceback
  unsigned long long* ext_bitmap = nullptr;
  uint32_t ext_q = 0;
  hipEvent_t ext_wait = nullptr;
  // per-text mode: the chunk descriptors come from the caller (one per text of a block-aligned
  // multi-text buffer); no prefilter, no chunk builder -- list DP -> rank -> traceback
  const ChunkDesc* ext_desc = nullptr;
  uint32_t ext_ndesc = 0;
  // both strands from one pass (whole texts): the prefilter of this, the forward strand's, job also
  // evaluates the Rc strand's pattern rc_pat (= complement(pattern)) on the forward text and marks
  // rc_bitmap in the coordinates of the reversed text; rc_marked tells whether the chosen filter did
  // (bit-plane and counting filters do).  The Rc job then takes that bitmap as ext_bitmap and reads
  // the forward buffer backwards (rev_n = its length): no reversed copy exists.
  unsigned long long* rc_bitmap = nullptr;
  const uint8_t* rc_pat = nullptr;
  bool rc_marked = false;
  bool rc_second_pass = false;       // more than 4 pieces: the Rc pieces get their own filter launch
  ScanParams F2{};
  uint64_t rev_n = 0;
  bool signal_filter_done = false;   // pipelining: record L.ev_filter_done behind this filter
  uint8_t* ctl_base = nullptr;       // this search's control block (the lane's d_ctl or its twin)
  bool ctl_pre_cleared = false;      // ... whose first 64 bytes the previous search cleared
  bool wait_ev_done = false;         // the host waits for L.ev_done (the twin's clear follows it in the stream)
  // shared pass (attempt 0 only): the launches that served this job (its own lane's or another's), in place of the whole
  // launch of enqueue_filter
  std::vector<PassSlot*> passes;
  bool group_ok() const;                    // this job can be a member of a grouped pass
  bool group_fits(const ScanJob& b) const;  // ... together with b (same buffer and launch geometry, <= 8 pieces)
  bool pipelined = false;            // one of several searches in flight (sassy_hip_search_shard_begin): the
                                     // bit-plane filter takes only half of a CU's wave slots, so that the previous
                                     // search's small tail kernels find room next to it

  static constexpr size_t kCtlHead = 64 + 4 * (size_t)kRankLimit;
  static constexpr uint32_t kTraceWaveMax = 8192;
  // list mode: longest chunk in blocks.  Long runs of candidate blocks (N runs under the Iupac profile,
  // low-complexity stretches) are cut there; every cut costs the next chunk wb warm-up blocks, every uncut run
  // is one lane walking it alone.  8 * wb blocks keep the warm-up at an eighth of the work (m = 32: 16-block
  // chunks, a 4 KiB N run is shared by four lanes instead of one).
  uint32_t maxlen = 128;
  static constexpr uint32_t kSpec = 4096;  // reports the kernels also write into the host buffer
  static constexpr size_t kPinCounts = 0, kPinCounters = 16, kPinFlags = 64;
  static constexpr size_t kPinFlags2 = 68, kPinCount2 = 72;  // dense results: the device's flag word and the count behind the dedup
  static constexpr size_t pin_cands = 128;
  static constexpr size_t pin_recs = pin_cands + (size_t)kSpec * sizeof(Candidate);
  static constexpr size_t pin_ops = pin_recs + (size_t)kSpec * sizeof(MatchOut);

  bool empty = false;
  double t_enter = 0, t_mark = 0;
  uint64_t n_blocks = 0, first_owned = 0, owned = 0, n_words = 0;
  ScanParams P{}, F{};
  uint32_t bucket = 4, q = 0;
  bool filtered = false;
  FilterKind fkind = kFilterGeneric;
  uint32_t count_r = 0, count_w = 0, count_t = 0, count_wpg = 4;  // counting filter: R, window blocks, threshold, waves per workgroup
  uint32_t pair = 0;                                   // paired filter: super-pieces (0: not taken)
  bool rows_declined = false;                          // the few-chunks list kernel found more chunks than it takes: the lane-per-chunk kernel runs them
  bool count_direct = false;                           // counting filter: it files the chunk descriptors itself (no bitmap, no chunk-list launch)
  double count_tail = 0;                           // ... and the expected fraction of candidate blocks
  unsigned long long* d_bitmap = nullptr;
  uint32_t* d_counts = nullptr;
  unsigned long long* d_counters = nullptr;
  TraceParams T{}, Tw{};
  uint32_t trace_blocks = 0, wave_blocks = 0, grid = 0, fgrid = 0, desc_cap = 0;
  bool use_wave = false, use_thread = false, ev_scan = false, self_rank = false, tuned = false;
  // fused: the bit-plane filter also runs the chunk DP (filter_dna_kernel<.., FUSED>): no bitmap, no chunk list, no
  // list kernel; no_fuse: this job already fell back to the classic chain
  bool fused = false, no_fuse = false;
  uint32_t counts[2] = {0, 0};  // reports, chunk descriptors
  int timing = 1;

  ScanJob(sassy_SearcherType* S_, ScanLane& L_, const ShardView& sh_, const PatternPlan& plan_, uint32_t k_,
          bool all_, const uint8_t* pat_, bool do_trace_, uint64_t total_len_)
      : S(S_), L(L_), sh(sh_), plan(plan_), k(k_), all_minima(all_), pat(pat_), do_trace(do_trace_),
        total_len(total_len_) {}
  int prepare();
  // enqueue = head (buffers, control block, what the filter launch reads), the search's own whole filter launch, tail
  // (everything behind the filter).  The shared pass calls head and tail itself and serves the job with enqueue_pass
  // launches in between (with_group_event: another lane's launch will read this lane's control block and tables).
  int enqueue(int attempt);
  int enqueue_head(int attempt, bool with_group_event = false);
  int enqueue_filter(int attempt);
  int enqueue_tail(int attempt);
  // the fused filter over the workgroups [g0, g1) for this job alone (the G = 1 launch) or with `other` (the G = 2
  // launch) on this job's lane; slot: the launch's events
  // (kept: where the launch's code planes come from -- the searcher's store, behind the events in kept->wait)
  struct KeptPlanes {
    int source = kPlaneRaw;
    uint4* store = nullptr;
    uint64_t store_bytes = 0;
    hipEvent_t wait[2] = {nullptr, nullptr};
  };
  int enqueue_pass(ScanJob* other, uint32_t g0, uint32_t g1, PassSlot& slot, const KeptPlanes* kept = nullptr);
  int finish(ScanOut& out);
  int finish_once(ScanOut& out, bool& redo);
};

// Several independent scans (different patterns over the same resident buffer) in flight, one per
// lane: while the GPU runs one pattern's kernels the host already queues the next one's and unpacks
// the previous one's results.  submit() blocks only when every lane is busy; results come back in
// submission order through the callback.
struct ScanQueue {
  struct Slot {
    PatternPlan plan;
    std::vector<uint8_t> pat;
    std::unique_ptr<ScanJob> job;
    uint64_t tag = 0;
    bool busy = false;
  };
  typedef std::function<int(uint64_t tag, ScanOut& so, const PatternPlan& plan, const uint8_t* pat)> Done;
  sassy_SearcherType* S;
  int n_lanes;
  Slot slots[kMaxLanes];
  int head = 0, tail = 0, in_flight = 0;  // ring over the lanes
  bool inputs_marked = false;
  Done done;

  ScanQueue(sassy_SearcherType* S_, Done d) : S(S_), done(std::move(d)) {
    n_lanes = kMaxLanes;
  }
  int drain_one() {
    Slot& sl = slots[head];
    ScanOut so;
    int rc = sl.job->finish(so);
    sl.job.reset();
    sl.busy = false;
    head = (head + 1) % n_lanes;
    --in_flight;
    if (rc) return rc;
    return done(sl.tag, so, sl.plan, sl.pat.data());
  }
  int drain_all() {
    int first = 0;
    while (in_flight) {
      const int rc = drain_one();
      if (rc && !first) first = rc;
    }
    return first;
  }
  int submit(const PatternPlan& plan, const uint8_t* pat, const ShardView& sh, const TextTable& texts, uint32_t k,
             bool all_minima, bool do_trace, uint64_t total_len, uint64_t tag, unsigned long long* ext_bitmap = nullptr,
             uint32_t ext_q = 0, hipEvent_t ext_wait = nullptr, const ChunkDesc* ext_desc = nullptr,
             uint32_t ext_ndesc = 0) {
    if (in_flight == n_lanes)
      if (int rc = drain_one()) return rc;
    if (!inputs_marked) {
      // text uploads / the reverse kernel of this call were queued on the searcher's stream: every
      // other lane waits for them once
      HIP_TRY(hipEventRecord(S->ev_inputs, S->stream));
      for (int l = 1; l < n_lanes; ++l) HIP_TRY(hipStreamWaitEvent(S->lanes[l].stream, S->ev_inputs, 0));
      inputs_marked = true;
    }
    Slot& sl = slots[tail];
    sl.plan = plan;
    sl.pat.assign(pat, pat + plan.m);
    sl.tag = tag;
    sl.job.reset(new ScanJob(S, S->lanes[tail], sh, sl.plan, k, all_minima, sl.pat.data(), do_trace, total_len));
    sl.job->texts = texts;
    sl.job->texts.all_minima = all_minima ? 1u : 0u;
    sl.job->ext_bitmap = ext_bitmap;
    sl.job->ext_q = ext_q;
    sl.job->ext_wait = ext_wait;
    sl.job->ext_desc = ext_desc;
    sl.job->ext_ndesc = ext_ndesc;
    ScanJob& job = *sl.job;
    // the slot counts as in flight only once its kernels are queued: a job whose prepare() / enqueue()
    // failed must never reach finish() (it would read the lane's previous counts and re-run on
    // half-initialised parameters)
    int rc = job.prepare();
    if (rc == 0 && !job.empty) rc = job.enqueue(0);
    if (rc != 0) {
      (void)hipStreamSynchronize(S->lanes[tail].stream);  // whatever part of it was queued
      sl.job.reset();
      return rc;
    }
    sl.busy = true;
    tail = (tail + 1) % n_lanes;
    ++in_flight;
    return 0;
  }
  ~ScanQueue() {  // never leave work in flight behind an error return
    while (in_flight) {
      ScanOut so;
      (void)slots[head].job->finish(so);
      slots[head].job.reset();
      head = (head + 1) % n_lanes;
      --in_flight;
    }
  }
};

// Host view of a multi-text buffer (see TextTable in common.h).  Null = the buffer is one text.
struct HostTexts {
  std::vector<uint64_t> start, len;
};
// [ts, te) of the text report c belongs to, in buffer coordinates
inline void text_bounds(const HostTexts* ht, const Candidate& c, uint64_t total_len, uint64_t& ts, uint64_t& te,
                               uint64_t& text_idx) {
  if (ht) {
    text_idx = c.flags >> kCandTextShift;
    ts = ht->start[text_idx];
    te = ts + ht->len[text_idx];
  } else {
    text_idx = 0;
    ts = 0;
    te = total_len;
  }
}

// Searcher::search / search_all on one text (reference: src/search.rs:510-525, 685-700, 787-881).
// `text` is a host pointer unless TEXT_ON_DEVICE.
// End-position callback of search_with_fn (reference: src/search.rs:767-784, applied at :895-906).
struct EndFilter {
  sassy_hip_end_filter fn = nullptr;
  void* user = nullptr;
};

// The tail of the one-pass searches of many patterns (pattern-tiled scan, seeded search): d_tiled_list holds
// `count` records (pattern, end position, cost) -- EVERY end position with cost <= k of every pattern, in any
// order, `copies`: possibly several times.  Sort by (pattern, position), apply the report rule to each run
// (sort_kernels.hip), trace the reports with one wavefront each (the report's pattern comes with it), apply the
// searcher's report filters per pattern and append the records to R.
// tt / ht: the buffer holds several texts (device / host tables): a report learns its text from its position,
// reports inside a separator are moved to their text's end (search_all: dropped), the records carry text-relative
// coordinates and the text's index in the buffer.
// defer (search_many over a batch of texts, traced, no report filters, not search_all): the records stay on the
// device -- in the buffers of lane defer->lane -- for assemble_many, nothing is appended to R.
struct ManyDefer {
  int lane = 0;
  ManyPart part{nullptr, nullptr, 0};
  uint32_t str_stride = 0;
};
inline void reset_stats(sassy_SearcherType* S) {
  S->stats = sassy_hip_Stats{};
  S->stats.pass_patterns = 1;
}
// The synchronous entry points use the searcher's lanes (streams, device buffers, pinned result areas) themselves:
// with a ticket open they would overwrite what its finish() is going to read.
inline bool tickets_open(const sassy_SearcherType* s) {
  for (const sassy_hip_Ticket* t : s->lane_ticket)
    if (t) return true;
  return false;
}
// Runs the rest of the scope on the searcher's device and restores the thread's current device afterwards.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(sassy_SearcherType* s) {
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); return; }
    if (s->device < 0) s->device = cur;  // first use binds the searcher
    s->bound = true;
    if (s->device != cur && hipSetDevice(s->device) == hipSuccess) prev = cur;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
#define SASSY_NO_TICKETS(s)                                                                                              \
  do {                                                                                                                   \
    if (tickets_open(s))                                                                                                 \
      return fail(SASSY_HIP_EINVAL, "searches are in flight on this searcher (sassy_hip_search_shard_begin): finish them first"); \
  } while (0)

// SASSY_HIP_LINE_SPANS is sassy_hip_search's alone
#define SASSY_NO_LINE_SPANS(flags)                                                                                       \
  do {                                                                                                                   \
    if ((flags) & SASSY_HIP_LINE_SPANS)                                                                                  \
      return fail(SASSY_HIP_EUNSUPPORTED, "SASSY_HIP_LINE_SPANS is a flag of sassy_hip_search only");                    \
  } while (0)

// ---- the Hamming scan of one launch group over ranges of tiles (hamming.hip), shared with amplicons.hip ----
// (HamItem, HamPattern, HamGroup, HamTables and every decision that needs no device: hamming_plan.h)
static_assert(sizeof(HamItem) == sizeof(Candidate) && offsetof(Candidate, pos) == 0, "items are sorted as candidates");
static_assert(kHamSlots == (uint32_t)kMaxSlots, "a launch's slots are ScanParams::slot_val");
// The text on the device, readable up to the next multiple of 64 bytes: one text, or -- starts != nullptr -- a laid-out batch.
struct HamText {
  const uint8_t* d_text = nullptr;
  uint64_t n = 0;        // bytes (a batch: of the whole buffer)
  uint64_t longest = 0;  // the longest text: n, or the batch's
  // a batch (device pointers): per block the bytes left in its own text, per text its first byte; the first text's index in the call
  const uint32_t* rem = nullptr;
  const uint64_t* starts = nullptr;
  uint32_t n_texts = 0;
  uint64_t text0 = 0;
  uint64_t n_blocks() const { return (n + 63) / 64; }
  uint64_t n_tiles() const { return (n_blocks() + kHamTileBlocks - 1) / kHamTileBlocks; }
};
// What the caller names: the group's patterns -- all[group.a0 .. group.a1) --, the text, the threshold.
struct HamJob {
  const HamPattern* pats = nullptr;  // the group's first
  uint32_t np = 0;
  HamGroup group;
  HamText text;
  uint32_t k = 0;
  uint64_t min_span = 1;  // a range is never cut below this many tiles: it overflows instead
};
// What ham_prepare leaves, once per group: the tables as built and where they are on the device, the kernels' slot values, the
// item list's size (ham_scan_range grows it).
struct HamPrepared {
  HamTables t;
  ScanParams SP{};
  uint32_t *d_tab = nullptr, *d_rows = nullptr;
  uint8_t* d_pats = nullptr;
  uint64_t item_cap = 0;
};
// What one range returns: the tiles scanned, their items sorted by (pattern | strand, block) -- here and in S->d_ham_sorted.
struct HamRangeOut {
  uint64_t span = 0;
  uint32_t count = 0;
  std::vector<HamItem> items;
  bool overflow = false;  // min_span tiles do not fit the list at its cap: nothing was scanned
};

// ---- functions one unit calls in another ----
// hamming.hip
int ham_prepare(sassy_SearcherType* S, const HamJob& J, HamPrepared& P);
int ham_scan_range(sassy_SearcherType* S, const HamJob& J, HamPrepared& P, uint64_t tile0, HamRangeOut& out);
// what every Hamming entry point refuses, before any device work; `who` names the entry point
int hamming_refusals(sassy_SearcherType* s, const uint8_t* const* pats, const size_t* lens, size_t n_pats, size_t k, const char* who);
// The drivers over a read batch that is resident and laid out (fastq_reads.hip's handle as one HamText with text0 = 0; `device`:
// where it was made, another one than the searcher's is SASSY_HIP_EINVAL): records in the contract's order, the best-pattern
// cells on the host, the counts table.  The first two stand behind the caller's hamming_refusals, the third calls it.
int hamming_reads_records(sassy_SearcherType* s, const uint8_t* const* pats, const size_t* lens, size_t n_pats, const HamText& reads, int device,
                          size_t k, bool without_trace, sassy_hip_Result* R);
int hamming_reads_cells(sassy_SearcherType* s, const uint8_t* const* pats, const size_t* lens, size_t n_pats, const HamText& reads, int device,
                        size_t k, unsigned long long* cells);
int hamming_reads_counts(sassy_SearcherType* s, const uint8_t* const* pats, const size_t* lens, size_t n_pats, const HamText& reads, int device,
                         size_t k, const char* who, uint64_t* out_counts);
// A group's tiles in ranges, for the callers that list records: every range asks for all that is left and ham_scan_range cuts
// it to what the item list holds.  per_range(range, t1, last, &next) makes the records of tiles [.., t1) and may move `next`,
// the tile the next range starts at (t1 as it comes).  Each range's records come in the contract's order and the ranges
// ascend, so behind more than one range reorder() -- a stable sort of the group's records -- restores it.
template <typename PerRange, typename Reorder>
int ham_walk_ranges(sassy_SearcherType* S, const HamJob& J, HamPrepared& P, PerRange&& per_range, Reorder&& reorder) {
  const uint64_t n_tiles = J.text.n_tiles();
  HamRangeOut range;
  uint32_t ranges = 0;
  for (uint64_t tile0 = 0;;) {
    if (int rc = ham_scan_range(S, J, P, tile0, range)) return rc;
    const uint64_t t1 = tile0 + range.span;
    const bool last = t1 >= n_tiles;
    uint64_t next = t1;
    if (int rc = per_range(range, t1, last, &next)) return rc;
    ++ranges;
    if (last) break;
    tile0 = next;
  }
  if (ranges > 1) reorder();
  return 0;
}
// `recs` records of a range in batches of the record block (option hamming_records): reserve(batch) sizes the device buffers
// once, emit(first, count) launches, downloads and appends.
template <typename Reserve, typename Emit>
int ham_emit_batches(const sassy_SearcherType* S, uint64_t recs, Reserve&& reserve, Emit&& emit) {
  const uint64_t batch = std::min<uint64_t>(recs, S->sw.hamming_records > 0 ? (uint64_t)S->sw.hamming_records : (1u << 20));
  if (int rc = reserve(batch)) return rc;
  for (uint64_t r0 = 0; r0 < recs; r0 += batch)
    if (int rc = emit(r0, (uint32_t)std::min<uint64_t>(batch, recs - r0))) return rc;
  return 0;
}
// What a Hamming entry point does around its device work, behind its refusals: the device, fresh stats, k cut to the longest
// pattern (k >= m takes every start), run(k), a stream sync where that failed, total_ms.
template <typename Run>
int hamming_call(sassy_SearcherType* s, const size_t* lens, size_t n_pats, size_t k, Run&& run) {
  DeviceGuard on_device(s);
  const double t0 = now_ms();
  reset_stats(s);
  if (int rc = s->ensure_device()) return rc;
  size_t longest = 0;
  for (size_t i = 0; i < n_pats; ++i) longest = std::max(longest, lens[i]);
  if (int rc = run((uint32_t)std::min<size_t>(k, longest))) {
    (void)hipStreamSynchronize(s->stream);
    return rc;
  }
  s->stats.total_ms = now_ms() - t0;
  return 0;
}
// hamming_pairs.hip, shared with edit_pairs.hip: what a pair call does behind its survey (one PairsCell per chunk and entry,
// cells[chunk][entry]) whatever the distance -- the rows' places and their 64-bit scan, the records' way back, the nearest
// fold, the pass times.  The kernels exist once, in hamming_pairs.hip.
int pairs_place_rows(sassy_SearcherType* s, uint4* cells, uint64_t n_a, uint32_t n_chunks, const unsigned long long** row_first_out,
                     unsigned long long* total_out);
int pairs_take_records(sassy_SearcherType* s, unsigned long long total, sassy_hip_HammingPair** out, size_t* n_out);
int pairs_fold_nearest(sassy_SearcherType* s, const uint4* cells, uint64_t n_a, uint32_t n_chunks, uint32_t S, uint8_t* out_cost, uint32_t* out_index,
                       uint8_t* out_strand, uint32_t* out_ties);
void pairs_times(sassy_SearcherType* s, bool has_last);
void pairs_for_slices(size_t n, const std::function<void(size_t, size_t)>& slice);  // the lists' encoding, in host threads
// A pair entry point's body: what throws for want of host memory (the lists' tables and planes are sized by the caller's n)
// comes back as SASSY_HIP_ENOMEM.
template <typename Body>
int pairs_guarded(const char* who, Body&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail(SASSY_HIP_ENOMEM, std::string(who) + ": out of host memory");
  } catch (const std::length_error&) {
    return fail(SASSY_HIP_ENOMEM, std::string(who) + ": out of host memory (a list too long for a host table)");
  }
}
// The clustering calls (clusters.hip; DESIGN.md 5.10 "Clusters").  Their refusals are the self-mode pair calls' own (b == NULL),
// defined next to those calls; each pair unit has one launcher that encodes and uploads the list, plans as its pair call
// does and links {i, j} in `d_parent` (device, n entries, parent[i] = i) for every pair of its walk's self-mode triangle --
// the events ev_line[0] and [1] around the link kernel, the stats' geometry filled in.
int pairs_refusals(sassy_SearcherType* s, bool have_out, const uint8_t* a, size_t n_a, const uint8_t* b, size_t n_b, size_t m, size_t k, uint32_t flags,
                   const char* who);
int edit_refusals(sassy_SearcherType* s, bool have_out, const uint8_t* a, size_t n_a, size_t m_a, const uint8_t* b, size_t n_b, size_t m_b, size_t k,
                  uint32_t flags, const char* who);
int pairs_link_components(sassy_SearcherType* s, const uint8_t* a, size_t n, uint32_t m, uint32_t k, uint32_t* d_parent);
// The UMI grouping call (umi_groups.hip; DESIGN.md 5.10 "UMI groups") walks device-resident arrays of the distinct sequences:
// the list's upload alone (*d_a [n][P W], *d_t [S n][P W]), the link pass and the record passes (survey, rows, scan, fill;
// the records stay in d_pairs_out) over such arrays, and the 64-bit exclusive scan the record passes use.
int pairs_upload_self(sassy_SearcherType* s, const uint8_t* a, size_t n, uint32_t m, const uint32_t** d_a, const uint32_t** d_t);
int pairs_resident_link(sassy_SearcherType* s, const uint32_t* d_a, const uint32_t* d_t, size_t n, uint32_t m, uint32_t k, uint32_t* d_parent);
int pairs_resident_records(sassy_SearcherType* s, const uint32_t* d_a, const uint32_t* d_t, size_t n, uint32_t m, uint32_t k, const char* who,
                           unsigned long long* total);
// umi_groups.hip, for dedup_reads.hip: the grouping call behind the list's upload, over planes that lie on the device
// (d_planes [n][P W]; d_targets [S n][P W], read by an rc searcher only).  out_label == NULL: no column is copied back and
// *n_groups is not counted.  *dev: the four columns on the device, n entries each, until the searcher's next grouping call.
struct UmiColumns {
  const uint32_t *label, *size, *rep, *count;
};
int umi_groups_resident(sassy_SearcherType* s, const uint32_t* d_planes, const uint32_t* d_targets, size_t n, uint32_t m, uint32_t k, uint32_t method,
                        uint32_t* out_label, uint32_t* out_size, uint32_t* out_rep, uint32_t* out_count, size_t* n_unique, size_t* n_groups,
                        UmiColumns* dev);
uint64_t pairs_scan_blocks(uint64_t n);
int pairs_scan_u64(sassy_SearcherType* s, const unsigned long long* in, uint64_t n, unsigned long long* block_sum, unsigned long long* out);
int edit_link_components(sassy_SearcherType* s, const uint8_t* a, size_t n, uint32_t m, uint32_t k, uint32_t* d_parent);
// cluster_step.h's memory policy on the device: relaxed, agent scope, vector memory operations
struct ClusterDeviceMem {
  uint32_t* parent;
  __device__ __forceinline__ uint32_t load(uint32_t x) const { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ bool cas(uint32_t x, uint32_t expect, uint32_t desired) const {
    return __hip_atomic_compare_exchange_strong(parent + x, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
// The one text of search_hamming, hamming_counts and hamming_amplicons on the device: the caller's device pointer, or an upload.
inline int ham_one_text(sassy_SearcherType* s, const void* text, size_t text_len, uint32_t flags, HamText* out) {
  const uint8_t* d_text = static_cast<const uint8_t*>(text);
  if (flags & SASSY_HIP_TEXT_ON_DEVICE) {
    if (((uintptr_t)text & 15) != 0) return fail(SASSY_HIP_EINVAL, "device text pointer must be 16-byte aligned");
  } else if (text_len) {
    if (int rc = s->d_text.reserve(text_len + 64)) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_text.p, text, text_len, hipMemcpyHostToDevice, s->stream));
    d_text = s->d_text.p;
  }
  *out = HamText{d_text, text_len, text_len};
  return 0;
}
// line_index.hip
int line_spans_on_device(sassy_SearcherType* S, const uint8_t* d_text, uint64_t text_len, const uint64_t* first, const uint64_t* last,
                         size_t n, sassy_hip_LineSpan* out);
struct TiledPerText;  // (many_patterns.hip)
// c_abi.hip
bool parse_alphabet(const char* alphabet, Profile& pr);
// Where the texts of a search_many call come from: the caller's pointers -- host memory, or device memory under
// SASSY_HIP_TEXT_ON_DEVICE --, or a read batch resident on the device (`reads`; then texts[r] = its d_text + seq_start[r],
// device pointers for the general path, lens[r] = seq_len[r] from its record table, and the flag is set).  The one-pass
// paths lay a batch of host texts out on the host and upload it (layout_and_upload); a resident batch is laid out by
// reads_relayout.hip's kernel into the same buffer, byte for byte the same.
struct TextSource {
  const uint8_t* const* texts = nullptr;
  const size_t* lens = nullptr;
  size_t n = 0;
  const sassy_hip_Reads* reads = nullptr;
  int plain = -1;  // reads: does every sequence hold A, C, G, T only?  (-1: not looked at yet -- reads_plain)
};
// reads_relayout.hip
// Reads first .. first + count of the handle to d_dst + d_dst_start[i] (a device table), every other byte of [0, total) = pad.
int reads_relayout(const sassy_hip_Reads* reads, uint64_t first, uint64_t count, const uint64_t* d_dst_start, uint64_t total, uint8_t pad,
                   uint8_t* d_dst, hipStream_t stream);
// acgt_only over every sequence of the handle, on the device, once per source
int reads_plain(sassy_SearcherType* s, TextSource& src, bool* plain);
// The handle as a text source: what every *_reads sibling of the search_many family refuses (reads == NULL, the flag
// SASSY_HIP_TEXT_ON_DEVICE, open tickets, another device than the searcher's), then the pointers and lengths.
struct ReadsTexts {
  std::vector<const uint8_t*> ptr;
  std::vector<size_t> len;
  TextSource src;
};
int reads_as_source(sassy_SearcherType* s, const sassy_hip_Reads* reads, uint32_t flags, const char* who, ReadsTexts* out);
// reads_call.hip: what surrounds the refusal predicate of every call on a resident read batch (reads_gate.h).
// The gate off the searcher and the handles as pointers (s may be NULL; r2 == NULL with handles == 1) ...
ReadsGate reads_gate_of(const sassy_SearcherType* s, uint32_t handles, const sassy_hip_Reads* r1, const sassy_hip_Reads* r2);
// ... and off the handles themselves, once nothing in front of them is wrong (first use binds the searcher to the thread's device)
void reads_gate_read(sassy_SearcherType* s, const sassy_hip_Reads* r1, const sassy_hip_Reads* r2, ReadsGate* g);
// What a refusal of the gate says and returns in the call `name`; the sentences that are the call's own come with it.
struct ReadsWho {
  const char *name, *ascii, *overhang, *only_best;
};
int reads_refused(ReadsRefusal why, const ReadsGate& g, const ReadsWho& who);
// The Dna look: a dna searcher takes reads of A, C, G, T only (reads_plain, on the device).  The refusal reads
// "<who>: <subject> other bytes than A, C, G, T, which a dna searcher cannot <verb>: use an iupac searcher".  *launches, where
// given, grows by the look's kernel where it ran.
int reads_require_plain(sassy_SearcherType* s, const sassy_hip_Reads* reads, const char* who, const char* subject, const char* verb, uint32_t* launches);
// sassy_hip_reads_slice and _select behind their own checks: record j of *out is [begins[j], +lens[j]) of read src[j] of `reads`
// (src == NULL: of read j; begins == NULL: whole reads), on the handle's device for the length of the call.
int windows_from_host(const sassy_hip_Reads* reads, const uint64_t* src, const uint64_t* begins, const uint64_t* lens, uint64_t n_out, hipStream_t st,
                      const char* who, sassy_hip_Reads** out);
// A call that returns a new resident batch, behind its refusals: hamming_call's frame (k cut to `longest`) around
// run(k, F), F a fresh handle on the searcher's device -- released where run fails, *out where it succeeds.  out == NULL: no
// handle is wanted, F == NULL.
template <typename Run>
int reads_new_batch(sassy_SearcherType* s, size_t longest, size_t k, sassy_hip_Reads** out, Run&& run) {
  std::unique_ptr<sassy_hip_Reads> F(out ? new sassy_hip_Reads : nullptr);
  const size_t lens[1] = {longest};
  const int rc = hamming_call(s, lens, 1, k, [&](uint32_t kk) {
    if (F) F->device = s->device;
    return run(kk, F.get());
  });
  if (rc != 0) {
    if (F) F->release();
    return rc;
  }
  if (out) *out = F.release();
  return 0;
}
// read_overlaps.hip, for merge_pairs.hip: the overlap call behind its refusals and inside the caller's frame (the Dna look,
// the kernel; k cut already).  The records stay in s->d_overlaps; they are copied to `out` only where it is given.
int overlaps_resident(sassy_SearcherType* s, const sassy_hip_Reads* r1, const sassy_hip_Reads* r2, uint32_t min_overlap, uint32_t k,
                      uint32_t max_permille, sassy_hip_ReadOverlap* out);
// ... and what a refusal of overlap_step.h's ovl_refusal says and returns in a call named `who`
int overlap_refused(uint32_t why, ReadsRefusal gate, const struct OvlCall& c, const char* who);
// fastq_reads.hip, for merge_pairs.hip: the layout of a new handle whose read r is the merged read of pair r (see there)
int reads_layout_merged(const sassy_hip_ReadOverlap* d_rec, const uint64_t* d_len1, const uint64_t* d_len2, uint64_t n, ScanLane* lane,
                        sassy_hip_Reads* F, uint64_t* n_merged);
// ... for trim_reads.hip: the layout of a new handle whose read r is as long as trim record r says, or as a table of window
// lengths says (see there)
int reads_layout_trimmed(const sassy_hip_ReadTrim* d_rec, uint64_t n, bool keep_quality, ScanLane* lane, sassy_hip_Reads* F, uint64_t* n_found);
int reads_layout_windows(const uint64_t* d_lens, uint64_t n, bool keep_quality, hipStream_t st, sassy_hip_Reads* F);
// trim_reads.hip, for demux_reads.hip too: the write kernel over a laid-out handle F (see there), and the buffers of a handle
// without a record
int write_windows(const sassy_hip_Reads* reads, const uint64_t* d_src, const uint64_t* d_begin, sassy_hip_Reads* F, hipStream_t st);
int reads_empty_buffers(sassy_hip_Reads* F, bool keep_quality, hipStream_t st);
// c_abi.hip: sassy_hip_search_many behind its null checks
int search_many_source(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens, size_t n_patterns, TextSource& src,
                       size_t k, uint32_t flags, sassy_hip_Result** out);
// many_patterns.hip
int search_many_batched(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens,
                               size_t n_patterns, TextSource& src, size_t k, uint32_t flags, sassy_hip_Result* R, bool& handled,
                               bool tiled_only = false);
double seeded_hit_rate(size_t m, size_t k);
double seeded_estimate(size_t m, size_t k, size_t n_patterns, uint64_t text_len);
int search_many_pertext(sassy_SearcherType* s, const uint8_t* const* patterns, const size_t* pattern_lens,
                               size_t n_patterns, TextSource& src, size_t k, uint32_t flags, sassy_hip_Result* R, bool& handled);
int search_encoded_tiled(sassy_SearcherType* s, const sassy_hip_Encoded* e, const uint8_t* tptr,
                                const uint8_t* h_text, uint64_t text_len, uint32_t k, bool all, bool wo,
                                sassy_hip_Result* R, bool* done, const TextTable* tt = nullptr,
                                const HostTexts* ht = nullptr, ManyDefer* defer = nullptr, const TiledPerText* pt = nullptr);
int search_encoded_seeded(sassy_SearcherType* s, const sassy_hip_Encoded* e, const uint8_t* tptr,
                                 const uint8_t* h_text, uint64_t text_len, uint32_t k, bool all, bool wo,
                                 sassy_hip_Result* R, bool* done, const TextTable* tt = nullptr,
                                 const HostTexts* ht = nullptr, bool dirty_text = false, ManyDefer* defer = nullptr,
                                 const TiledPerText* ov = nullptr);
int search_encoded_overhang(sassy_SearcherType* s, const sassy_hip_Encoded* e, const uint8_t* tptr, const uint8_t* h_text,
                            uint64_t text_len, uint32_t k, bool all, bool wo, sassy_hip_Result* R, bool* done);
bool many_tiled_wanted(const sassy_SearcherType* s, const size_t* pattern_lens, size_t n_patterns, uint64_t total, size_t k);
bool acgt_only(const uint8_t* p, size_t n);
// min_costs.hip
int reduce_pattern_list(sassy_SearcherType* s, uint32_t count, const TextTable* tt);
// scan_driver.hip
int stream_geometry(ScanParams& P, uint64_t owned, uint32_t extra_front, uint32_t* grid, int wpc = 16,
                    GeoTuner* tuner = nullptr, const void* tune_text = nullptr, uint64_t tune_len = 0, uint32_t tune_kind = 0);
int post_filter(sassy_SearcherType* S, ScanOut& so, const PatternPlan& plan, const uint8_t* pat, uint32_t k,
                       int strand, const uint8_t* h_text, const uint8_t* d_text, uint64_t tlen, bool with_trace,
                       const EndFilter& ef, const HostTexts* ht = nullptr);
int append_matches(ScanOut& so, uint64_t total_len, const PatternPlan& plan, bool without_trace,
                          uint64_t pattern_idx, sassy_hip_Result* R, size_t& first, const HostTexts* ht = nullptr);
int layout_and_upload(uint8_t* dst, uint8_t* d_dst, const uint8_t* const* texts, const size_t* lens,
                             const uint64_t* start, size_t nt, uint64_t total, uint8_t pad, hipStream_t stream);
void layout_texts(uint8_t* dst, const uint8_t* const* texts, const size_t* lens, const uint64_t* start, size_t nt,
                         uint64_t total, uint8_t pad);
int search_text(sassy_SearcherType* S, const uint8_t* pattern, size_t plen, const uint8_t* text,
                       size_t tlen, size_t k, uint32_t flags, uint64_t pattern_idx, bool fwd_strand,
                       bool rc_strand, sassy_hip_Result* R, const EndFilter& ef = EndFilter(),
                       bool already_uploaded = false, const PatternPlan* class_plan = nullptr);
int run_scan(sassy_SearcherType* S, const ShardView& sh, const PatternPlan& plan, uint32_t k,
                    bool all_minima, const uint8_t* pat, bool do_trace, uint64_t total_len, ScanOut& out);
int run_scan_ref_lanes(sassy_SearcherType* S, const uint8_t* d_text, uint64_t n, const PatternPlan& plan, uint32_t k,
                              bool all_minima, const uint8_t* pat, bool do_trace, uint32_t lanes, ScanOut& out);
uint64_t required_halo_bytes(size_t pattern_len, size_t k);


}  // namespace sassy_hip
