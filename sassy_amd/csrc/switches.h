// switches.h -- every path-forcing / tuning switch of libsassy_hip.so, in ONE table.
//
// A searcher reads the table once, when it is created (sassy_hip_searcher_new, the workers of sassy_hip_multi_new): every
// entry takes its default, then the value of the environment variable SASSY_HIP_<NAME> if that is set; afterwards
// sassy_hip_set_option(searcher, "<name>", value) changes one entry of that searcher.  No search entry point reads the
// environment.  The switches exist for the parity tests (tests/test_gpu_parity.py: every entry is forced by a test named
// in DESIGN.md 5.7) and for the timing tools under tools/; a production caller needs none of them.
#pragma once
#include <cstdint>
#include <string>

namespace sassy_hip {

// X(field, default, "what it does")
#define SASSY_HIP_SWITCHES(X)                                                                                               \
  X(prefilter, -1, "-1: a prefilter where its pieces are selective; 0: never (streaming DP over every block); 1: also with 2-row pieces") \
  X(fused, 1, "the bit-plane filter runs the chunk DP of what it finds in the same launch (0: bitmap -> chunk list -> list kernel)") \
  X(ref_lanes, 0, "4 / 8: reproduce the reference binary's 4- / 8-lane reports on a single text (0: the one-pass definition)") \
  X(pipe_depth, 2, "searches in flight per searcher (1 .. 4) for search_shard_begin / _finish")                          \
  X(tune, 0, "1: the on-line geometry tuner tries neighbouring lane-chunk lengths during a resident text's first searches") \
  X(timing, 1, "HIP-event timing: 0 none, 1 the dominant kernel, 2 every phase")                                            \
  X(row_cut, 1, "0: the DP kernels compute every pattern row of every block (no wave-voted stop)")                         \
  X(filter_kind, 0, "force a prefilter kernel where it applies: 1 slot masks, 2 bit planes, 3 q-gram table, 4 q-gram counting") \
  X(self_rank, 1, "0: separate rank kernels instead of the traceback waves ranking their reports themselves")               \
  X(trace_wave, 1, "0: thread-per-report traceback only")                                                                   \
  X(iupac_planes, 1, "0: Iupac searchers with plain patterns take the Iupac chain, never the bit-plane launch with the text check") \
  X(short_pieces, 1, "0: no fused launch for shapes whose pigeonhole pieces are 6 rows")                                    \
  X(pair, 1, "0: no paired filter; 2: the counting filter keeps the shapes it is selective for")                            \
  X(pair_rc, 1, "0: both strands of a paired-filter shape through the forward strand's streaming DP with Rc marks")         \
  X(count_wpg, 0, "counting filter: waves per workgroup, 4 or 16 (0: by LDS fit)")                                          \
  X(count_fused, 1, "the counting filter hands its candidate blocks to the chunk DP without bitmap and chunk-list launch (0: classic chain)") \
  X(fused_probe, 0, "1: the fused launch reports where its waves spend their time; 2: no chunk DP at all (timing only, no reports)") \
  X(fused_press, 0, "> 0: a wave of the fused launch runs a chunk-DP pass once this many windows are queued")              \
  X(list_words, 1, "multi-word chunk DP of few chunks: 1 a lane per block (list_rows_kernel), 2 a lane per pattern word, 0 the lane-per-chunk kernel only")                                              \
  X(trace_threads, 0, ">= 64: threads of the thread-per-report traceback launch")                                           \
  X(trace_probe, 0, "1: the traceback waves report microseconds per phase to stderr")                                       \
  X(big_pin, 1, "0: dense results through the host's vectors instead of one pinned block")                                  \
  X(compact_cigars, 1, "0: dense results keep their cigar slots' padding")                                                  \
  X(adopt, 1, "0: results are copied out of the pinned block the kernels wrote them into")                                  \
  X(rc_fused, 1, "0: the Rc strand from a reversed copy instead of Rc marks made by the forward pass")                      \
  X(strands_in_flight, 1, "0: two strands that are two searches run one after the other")                                   \
  X(encoded_trace_threads, -1, "search_encoded: threads of the dense traceback launch (-1: by result size)")                \
  X(encoded_pin, 1, "0: search_encoded's dense results through the host's vectors")                                         \
  X(seed_layout, 1, "0: the seeded search cuts its seeds evenly instead of by expected table hits")                         \
  X(seed_subtest, 1, "0: seeded search without the sub-piece test")                                                         \
  X(seed_narrow, 1, "0: never the narrow (4-dword) sub-piece test layout")                                                  \
  X(seed_pos64, 0, "1: force the layout for positions beyond 32 bits")                                                      \
  X(many_tiled, -1, "search_many: 1 force / 0 forbid the one-pass paths (-1: by size)")                                     \
  X(many_seeded, -1, "search_many: 1 force / 0 forbid the seeded search inside the one-pass path")                          \
  X(many_assemble, 1, "0: search_many's records ordered by the host")                                                       \
  X(many_batch, 0, "> 0: a laid-out batch of search_many is at most this many bytes (a longer text is a batch of its own) (0: 1 GiB)") \
  X(overhang_tiled, 1, "0: overhang with many patterns as one launch per pattern and strand")                               \
  X(overhang_seeded, 1, "0: overhang with many patterns through the per-text tiled scan over everything")                   \
  X(multi_min_text, 16 << 20, "search_encoded: smallest text (bytes) for the multi-pattern prefilter")                       \
  X(tiled, -1, "search_encoded: 1 force / 0 forbid the pattern-tiled scan")                                                 \
  X(seeded, -1, "search_encoded: 1 force / 0 forbid the seeded search")                                                 \
  X(shared_pass, 1, "searches in flight over one buffer share text passes, two per fused bit-plane launch: 1 staggered in halves of the grid (a begin launches the previous search's second half with this one's first; a search with no partner and no pass streaming goes whole); 4: as 1, but a search without a partner always keeps its second half back; 0: a pass per search; 3: whole passes, a groupable search always waits for a partner; 2: as 3 while a pass streams, and a waiting search is launched before a finish that has to wait") \
  X(plane_cache, 1, "searches in flight keep the text's two code planes (16 bytes per 64-byte block, in a store per searcher) while tickets over one buffer are open without a break: the first launch over a half of the grid writes them, later ones read them instead of the text (0: every pass derives them from the text)") \
  X(plane_cache_max_mb, 0, "> 0: a plane store larger than this many MiB is not made (0: no cap)") \
  X(aa_batch, 0, "search_all_alignments: at most this many alignments per emit batch (0: 32 MiB of rows / cigar text)") \
  X(min_cost_device, 1, "min_costs / best_pattern: 0: never the device reduction of the scan's list (search_many's records reduced by the host)") \
  X(best_match_device, 1, "best_matches: 0: never the device path (locating reduction of the scan's list, one traceback per text); search_many's records reduced by the host") \
  X(hamming_items, 0, "search_hamming: > 0: the item list holds exactly this many 16-byte items (at least one tile's worth) and never grows -- a text range whose items overflow it is cut down and launched again (0: 65536, grown up to 4 Mi items before ranges are cut)") \
  X(hamming_records, 0, "search_hamming: > 0: records are emitted at most this many per launch of the emit kernel (0: 1 Mi)") \
  X(hamming_batch, 0, "search_hamming: > 0: at most this many scanned patterns (a strand counts as one) share a launch of the scan kernel (0: 512)") \
  X(hamming_many_batch, 0, "search_hamming_many / hamming_best_pattern: > 0: a batch of texts is at most this many bytes laid out (each text from a multiple of 64 on; a longer text is a batch of its own) (0: 1 GiB)") \
  X(hamming_count_copies, 0, "hamming_counts / hamming_counts_many: > 0: this many copies of the counts table -- a workgroup adds into copy blockIdx & (copies - 1), the host sums them (rounded down to a power of two, at most 1024) (0: 32 while 32 tables are at most 65536 counters, fewer for a larger table)") \
  X(pairs_chunks, 0, "hamming_pairs / hamming_nearest: > 0: the targets are cut into this many chunks (at most one per target, at most 65535) -- the grid is strips of 256 entries x chunks; geometry only (0: enough chunks of at least 256 targets that 2048 workgroups are in flight; hamming_pairs: also chunks of at most 16384 targets, within 2^24 partial cells)") \
  X(collapse_slots, 0, "umi_groups: > 0: the duplicate table holds this many slots, but at least one per read -- geometry only: at exactly one per read the table runs full and the probes wrap round (0: the power of two that is at least twice the reads)")

struct Switches {
#define SASSY_HIP_SWITCH_FIELD(name, dflt, doc) long name = (dflt);
  SASSY_HIP_SWITCHES(SASSY_HIP_SWITCH_FIELD)
#undef SASSY_HIP_SWITCH_FIELD
  // SASSY_HIP_DEVICES: the devices the drop-in search() of include/sassy.h fans a host text over ("all", or a list)
  std::string devices;
};

// defaults, then the environment (SASSY_HIP_<NAME in capitals>); the library's only reader of the environment
Switches load_switches();
// one entry by name (lower case, without the prefix); false: no such switch
bool set_switch(Switches& sw, const char* name, long value);
bool get_switch(const Switches& sw, const char* name, long* value);
// "name<TAB>default<TAB>what it does\n" per switch
const char* switch_table();

}  // namespace sassy_hip
