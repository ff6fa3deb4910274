/*
 * sassy_hip.h -- additive C-ABI of libsassy_hip.so (everything the reference exposes only
 * through its Rust API, plus the device-resident entry points the benchmark and the multi-GPU
 * driver need).  Plain pointers and sizes only; no torch / C++ types.
 *
 * Conventions: functions returning int return 0 on success and a negative code on error;
 * sassy_hip_last_error() then holds a message (thread-local).  Nothing here falls back to a CPU
 * implementation: without a usable HIP device the search calls fail with SASSY_HIP_ENODEVICE.
 */
#ifndef SASSY_HIP_H
#define SASSY_HIP_H

#include "sassy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SASSY_HIP_EINVAL (-1)    /* bad argument (null pointer, invalid pattern, ...) */
#define SASSY_HIP_ENODEVICE (-2) /* no usable HIP device / HIP runtime error */
#define SASSY_HIP_EUNSUPPORTED (-3)
#define SASSY_HIP_ENOMEM (-4)

/* search flags */
#define SASSY_HIP_ALL_MINIMA 1u     /* Searcher::search_all (src/search.rs:685-700) */
#define SASSY_HIP_WITHOUT_TRACE 2u  /* Searcher::without_trace (src/search.rs:448-451,1464-1475) */
#define SASSY_HIP_TEXT_ON_DEVICE 4u /* `text` is a device pointer (e.g. a torch tensor's data_ptr), 16-byte aligned; the
                                       kernels read whole 64-byte blocks: the allocation must be readable up to the
                                       next multiple of 64 bytes behind the text (any hipMalloc'ed buffer is -- a
                                       sub-range that ends exactly at the end of an allocation of a non-multiple size
                                       is not) */
#define SASSY_HIP_TEXT_UNCHANGED 8u /* with TEXT_ON_DEVICE: the bytes at `text` are the same as in this searcher's
                                       previous call with this pointer and length (many patterns, one resident
                                       text): the reversed copy the Rc strand scans is reused, not rebuilt */

#define SASSY_HIP_LINE_SPANS 16u    /* sassy_hip_search only: also resolve every match to the lines it lies in, while the text
                                       is still resident (sassy_hip_result_line_spans); every other call that takes flags
                                       refuses the bit with SASSY_HIP_EUNSUPPORTED, and so does sassy_hip_search together with
                                       SASSY_HIP_WITHOUT_TRACE (no match start to resolve) */
#define SASSY_HIP_KEEP_QUALITY 32u  /* sassy_hip_fastq_parse only: the handle also keeps the base qualities on the device, in
                                       the layout of its text (sassy_hip_reads_quality) */

/* Full match record = reference Match (src/search.rs:35-62).  cigar is the SAM text the
 * reference's Cigar::to_string gives ("3=1X"), stored in the result's string pool.
 * without_trace: text_start = pattern_start = UINT64_MAX and an empty cigar, as the reference. */
typedef struct sassy_hip_Match {
  uint64_t pattern_idx;
  uint64_t text_idx;
  uint64_t text_start;
  uint64_t text_end;
  uint64_t pattern_start;
  uint64_t pattern_end;
  int32_t cost;
  uint8_t strand; /* 0 = Fwd, 1 = Rc */
  uint8_t pad_[3];
  uint32_t cigar_off; /* offset of the NUL-terminated cigar string in the pool (the pool's bytes between the strings
                         are unspecified) */
  uint32_t cigar_len;
} sassy_hip_Match;

/* Where a span [first, last] of text positions lies, line-wise; '\n' (0x0A) is the only separator.  For a position p of a
 * text t of n bytes: line_no(p) = 1 + the number of '\n' in t[0:p]; line_start(p) = 1 + the index of the last '\n' in
 * t[0:p], 0 if there is none; line_end(p) = the index of the first '\n' in t[p:n], n if there is none.  The line of the
 * span is t[line_start:line_end) (without its '\n'); a span that contains newlines has last_line_no > line_no. */
typedef struct sassy_hip_LineSpan {
  uint64_t line_no;      /* line_no(first), 1-based */
  uint64_t last_line_no; /* line_no(last) */
  uint64_t line_start;   /* line_start(first) */
  uint64_t line_end;     /* line_end(last) */
} sassy_hip_LineSpan;
/* The line index counts newlines per tile of this many text bytes (sassy_hip_line_tile() returns the same). */
#define SASSY_HIP_LINE_TILE 4096u

typedef struct sassy_hip_Result sassy_hip_Result;       /* opaque, owns matches + cigar pool */
typedef struct sassy_hip_Encoded sassy_hip_Encoded;     /* opaque EncodedPatterns */

/* Per-call statistics of the last search on a searcher (for bench.py's roofline object). */
typedef struct sassy_hip_Stats {
  double scan_ms;        /* HIP-event time of the scan path (filter + chunk list + DP, or the streaming
                            scan), all strands; 0 unless timed (sassy_hip_set_timing) */
  double trace_ms;       /* HIP-event time of report ranking + traceback kernels (timing level 2) */
  double total_ms;       /* host wall time of the whole call */
  uint64_t text_bytes;   /* algorithmic bytes scanned (text_len per strand) */
  uint64_t scan_launches;
  uint64_t candidates;   /* (end_pos, cost) records produced by the scan */
  uint64_t cond_resolved;/* candidates whose plateau-entry direction needed the chunk-state chain */
  uint64_t chunks;       /* lane chunks the text was cut into */
  uint64_t blocks;       /* 64-byte text blocks visited incl. warm-up */
  uint64_t word_rows;    /* DP word-rows computed (0 unless the kernel was built with counters) */
  uint32_t blocks_per_chunk;
  uint32_t warmup_blocks;
  uint32_t grid;
  uint32_t filtered;     /* 0: DP over every block (scan_kernel); 1: prefilter (filter_kernel) -> chunk list ->
                            DP on the listed chunks; 2: the same with the Dna bit-plane prefilter (filter_dna_kernel);
                            3: q-gram piece table (filter_table_kernel); 4: q-gram counting (filter_count_kernel);
                            5: the pattern-tiled scan of search_encoded (tiled_kernel: all patterns in one pass);
                            6: the seeded search of search_encoded (seed_kernels: seed table lookups, one lane per hit);
                            7: the Hamming scan of sassy_hip_search_hamming (hamming.hip: no DP);
                            8: the all-vs-all walk of sassy_hip_hamming_pairs / _nearest (hamming_pairs.hip: no text);
                            9: the all-vs-all walk of sassy_hip_edit_pairs / _nearest (edit_pairs.hip: no text; also
                               where |m_a - m_b| > k and nothing was launched);
                            10: the link walk of sassy_hip_hamming_clusters (hamming_pairs.hip + clusters.hip: no text);
                            11: the link walk of sassy_hip_edit_clusters (edit_pairs.hip + clusters.hip: no text);
                            12: sassy_hip_umi_groups (umi_groups.hip: the collapse, then hamming_pairs.hip's walk over the
                                distinct sequences: no text); sassy_hip_umi_groups_reads and sassy_hip_dedup_reads as well
                                (dedup_reads.hip: the same device work over the windows of a resident read batch) */
  double filter_ms;      /* HIP-event time of the prefilter kernel (part of scan_ms); a search in flight whose text pass
                            was served by several launches (see pass_patterns): the sum of their durations */
  uint64_t hit_blocks;   /* text blocks in which an exact pattern piece ends */
  uint32_t piece_len;    /* rows per pattern piece (k+1 pieces) / q-gram length Q (filtered = 4), 0 when unfiltered */
  uint32_t fused;        /* 1: the bit-plane prefilter ran the chunk DP of what it found itself (one launch for
                            filter + chunk list + DP; sassy_hip_set_fused) */
  double host_enqueue_ms; /* host wall time spent queueing work on the stream */
  double host_wait_ms;    /* host wall time blocked in the stream synchronisation */
  double host_post_ms;    /* host wall time after it: sort, seams, cigar strings, result records */
  uint64_t live_blocks;   /* blocks whose last row passed the cheap "may hold a cell <= k" test and were
                             walked column by column (0 unless counters are enabled) */
  uint32_t pair;          /* != 0: the fused launch ran the PAIRED filter with this many super-pieces of 2 * piece_len
                             rows (one half exact, the other half with <= 1 edit next to it; SASSY_HIP_PAIR=0: never) */
  uint32_t pass_patterns; /* the largest number of searches a launch of this search's text pass served: 2 when a search
                             in flight shared one of them (sassy_hip_search_shard_begin), else 1 */
  uint32_t plane_launches; /* how many of the launches that served this search's text pass read the text's kept code
                              planes instead of the text (searches in flight, switch plane_cache); 0 for a lone search */
} sassy_hip_Stats;

const char *sassy_hip_last_error(void);
const char *sassy_hip_version(void);
int sassy_hip_device_count(void); /* number of visible HIP devices, 0 if none / no runtime */

/* Mirrors Searcher::new(rc, alpha) (src/search.rs:486-503) without aborting: NULL on error.
 * alpha = NAN: no overhang.  Otherwise (Iupac only, 0 <= alpha <= 1; src/search.rs:373-400) the
 * pattern may hang over either end of the text at alpha per overhanging character: matches then
 * carry pattern_start > 0 / pattern_end < pattern_len.  Overhang searches stream the full DP (the
 * pigeonhole prefilter does not cover partial patterns) and report nothing for an empty text. */
/* Alphabets: "dna", "iupac", "ascii" (src/c.rs:52-70) and "ascii_ci", in any letter case.  "ascii_ci" is the reference's
 * CaseInsensitiveAscii (src/profiles.rs:5): two bytes match iff u8::eq_ignore_ascii_case -- only A-Z and a-z fold, every
 * other byte (0x80-0xFF included) matches only itself -- in the scan and in the traceback alike.  It is accepted wherever
 * "ascii" is and behaves like it otherwise (no reverse complement, no overhang, the general search paths). */
sassy_SearcherType *sassy_hip_searcher_new(const char *alphabet, bool rc, float alpha);
/* The HIP device a searcher works on.  A searcher binds itself to the calling thread's current device at its first
 * search (HIP's current device is per host thread); sassy_hip_set_device chooses one before that.  From then on
 * every entry point runs on that device, whatever thread calls it, and restores the thread's current device
 * before it returns.  sassy_hip_get_device: -1 while unbound. */
int sassy_hip_set_device(sassy_SearcherType *s, int device);
int sassy_hip_get_device(const sassy_SearcherType *s);
/* Use an existing HIP stream (hipStream_t) for all work of this searcher; NULL = own stream. */
int sassy_hip_set_stream(sassy_SearcherType *s, void *hip_stream);
int sassy_hip_get_stats(const sassy_SearcherType *s, sassy_hip_Stats *out);
/* HIP-event timing behind the stats: 0 = none, 1 = the dominant kernel only (prefilter, or the
 * streaming scan when unfiltered; default), 2 = every phase (scan_ms, filter_ms, trace_ms).  Each
 * recorded event costs a few microseconds of stream idle time. */
int sassy_hip_set_timing(sassy_SearcherType *s, int level);
/* The switch table (sassy_amd/csrc/switches.h): every switch that forces a kernel path or sets a tuning
 * value.  A searcher fills its copy ONCE, when it is made: the defaults, then the environment variables
 * SASSY_HIP_<NAME> that are set -- no search entry point reads the environment.  sassy_hip_set_option changes one entry
 * of an existing searcher (name: lower case, without the prefix -- "fused", "filter_kind", "pair", ...; refused while
 * searches are in flight), sassy_hip_get_option reads one, sassy_hip_option_table returns "name<TAB>default<TAB>what it
 * does" lines for all of them.  All settings give the same matches: the switches exist so that every path can be
 * checked against the oracle (tests/test_gpu_parity.py) and timed apart (tools/). */
int sassy_hip_set_option(sassy_SearcherType *s, const char *name, long value);
int sassy_hip_get_option(const sassy_SearcherType *s, const char *name, long *value);
const char *sassy_hip_option_table(void);
/* Which scan path a searcher takes: -1 = the library's choice (exact prefilter where the pattern's pieces are
 * selective, the streaming DP otherwise; process-wide override: SASSY_HIP_PREFILTER), 0 = always the streaming
 * DP over every block, 1 = prefilter also with short pieces.  All give the same matches; the setting exists so
 * that the paths can be checked against each other (tests) and timed apart. */
int sassy_hip_set_prefilter(sassy_SearcherType *s, int mode);
/* The bit-plane prefilter (Dna, <= 8 pieces, one strand, one text) can finish the scan in its own launch: every
 * wavefront runs the chunk DP over the match-end blocks it found itself when it has streamed its text range
 * (no hit bitmap, no chunk-list kernel, no list kernel).  on = 1 (default; process-wide: SASSY_HIP_FUSED=0 turns it
 * off), 0 = always the classic chain.  Same matches either way; stats.fused tells which one ran.
 * An Iupac searcher takes the same launch when its pattern holds plain A C G T only (<= 4 pieces), on ANY text: the lane
 * that owns a block checks it for other letters and queues the columns a match touching them can end in; the chunk DP of
 * such a launch builds the Iupac profile's masks; the inside of a run of N is walked over, not searched (cost 0
 * everywhere: nothing to report under the report rule) -- SASSY_HIP_IUPAC_PLANES=0 turns the launch off.
 * What the fused launch cannot finish alone (a report on a long FLAT plateau of cost > 0 whose beginning no window
 * sees, a shard's exit state on such a plateau) sends that one search to the classic chain. */
int sassy_hip_set_fused(sassy_SearcherType *s, int on);
/* Which reports a search of ONE text returns on low-complexity text (sassy_hip_search, the drop-in search):
 * 0 (default) = the definition -- one left-to-right pass over the text, independent of any chunking;
 * 4 / 8 = what the reference binary built for AVX2 / AVX-512 returns: it cuts the text into 4 / 8 lanes that each
 * start with decreasing = true (src/search.rs:1016-1056, 1202-1240), which adds reports for <=k plateaus that
 * were entered by an increase left of a lane's start (never on random text).  Process default:
 * SASSY_HIP_REF_LANES.  Not applied with overhang, nor to shards.  search_many / search_encoded need no such
 * mode: with several patterns or texts the reference gives every lane a whole text (chunk_offset_blocks = 0,
 * src/search.rs:1034-1048; the v2 scan keeps a pattern per lane), so its reports ARE the definition's there. */
int sassy_hip_set_reference_lanes(sassy_SearcherType *s, int lanes);
/* On-line tuner of the streaming kernels' lane-chunk length for a resident text (off by default, or
 * SASSY_HIP_TUNE=1): the first ~36 searches of a (text, filter kind) try neighbouring geometries -- each a
 * complete, exact search -- and the rest use the fastest.  Worth it for the latency of lone searches on one
 * text at sizes where the default geometry is unlucky (up to 10 %); with searches in flight it moves the time
 * per search by 0-2 %. */
int sassy_hip_set_geometry_tuner(sassy_SearcherType *s, int on);
/* Count DP word-rows / blocks in the scan kernel (stats.word_rows, stats.blocks); off by default. */
int sassy_hip_enable_counters(sassy_SearcherType *s, int on);

/* Reporting modes of the reference's Searcher builder, applied per strand by sassy_hip_search,
 * sassy_hip_search_with_fn and sassy_hip_search_encoded (not by search_shard):
 *   only_best_match()  (src/search.rs:442-446, 1392-1412): one match per strand -- minimal cost,
 *                      rightmost end position;
 *   with_max_n_frac(f) (src/search.rs:454-475, src/n_filter.rs): drop matches whose text span holds
 *                      more than the fraction f of 'N'/'n'; f = 1.0 or NAN switches it off. */
int sassy_hip_set_only_best_match(sassy_SearcherType *s, int on);
/* Searcher::with_max_overhang (src/search.rs:436-440): at most this many overhanging characters are
 * priced with alpha (the rest cost 1 each); negative = no limit. */
int sassy_hip_set_max_overhang(sassy_SearcherType *s, long max_overhang);
int sassy_hip_set_max_n_frac(sassy_SearcherType *s, float max_n_frac);

/* Searcher::search / search_all with full Match records (src/search.rs:510-525, 685-700). */
int sassy_hip_search(sassy_SearcherType *s, const uint8_t *pattern, size_t pattern_len,
                     const uint8_t *text, size_t text_len, size_t k, uint32_t flags,
                     sassy_hip_Result **out);

/* Character-class patterns: position j of the pattern is a SET of byte values, 32 bytes per position -- byte value c belongs
 * to position j iff bit (c & 7) of sets[32 j + (c >> 3)] is set.  Cost is edit distance under "text byte is a member of
 * the row's set"; in the cigar '=' is a member and 'X' a non-member; an empty set is legal and matches nothing.  Flags,
 * records, cigar pool and report rule are those of sassy_hip_search (SASSY_HIP_ALL_MINIMA, _WITHOUT_TRACE,
 * _TEXT_ON_DEVICE, _TEXT_UNCHANGED, _LINE_SPANS).
 *  - the searcher's alphabet is "ascii" or "ascii_ci"; under ascii_ci every set is closed under the A-Z / a-z twin first;
 *  - a dna / iupac searcher, rc = true and an overhang searcher (alpha): SASSY_HIP_EUNSUPPORTED;
 *  - distinct sets are the pattern's profile slots: more than 64 distinct sets is SASSY_HIP_EINVAL;
 *  - every slot is covered by cubes (value, care) -- byte c is in a cube iff ((c ^ value) & care) == 0 --, each run of
 *    consecutive byte values by at most 14 aligned power-of-two cubes, the set or (complement flag) whichever of the
 *    set and its complement takes fewer: at most 128 per set.  The device builds a slot's match mask per 64-byte text
 *    block from its cubes, about 32 vector instructions per cube against 25 per pattern row; a pattern whose slots
 *    need more than SASSY_HIP_CLASS_MAX_CUBES cubes together is refused with SASSY_HIP_EINVAL rather than run slowly;
 *  - the search is the streaming DP over the whole text (no prefilter: their exactness rests on byte equality).
 * Not available for class patterns: search_all_alignments, search_many, min_costs, best_pattern, best_matches, encoded
 * patterns, shards / multi-device, search_with_fn -- those entry points take byte patterns only. */
#define SASSY_HIP_CLASS_MAX_CUBES 256
int sassy_hip_search_classes(sassy_SearcherType *s, const uint8_t *sets, size_t m, const void *text, size_t text_len, size_t k,
                             uint32_t flags, sassy_hip_Result **out);
/* The cover sassy_hip_search_classes gives one set (host only, no device needed): writes the first `cap` cubes to value[] /
 * care[], *complemented = 1 if they cover the set's complement, and returns the number of cubes (<= 128). */
long sassy_hip_class_cover(const uint8_t set[32], uint8_t *value, uint8_t *care, size_t cap, int *complemented);

/* Line resolution on the device (sassy_amd/csrc/line_index.hip): out[i] = the span of [first[i], last[i]] in the text, for
 * n spans with first[i] <= last[i] <= text_len (anything else: SASSY_HIP_EINVAL; last == text_len is the empty position
 * behind the text).  A match [text_start, text_end) is the span first = text_start, last = max(text_start, text_end - 1).
 * flags: SASSY_HIP_TEXT_ON_DEVICE (a device pointer as for sassy_hip_search) or 0 (the text is uploaded); first, last and
 * out are host arrays.  One pass over the text counts the newlines per tile, a second launch resolves all spans, one
 * wavefront each, at a cost that does not depend on the length of the lines.  n == 0: success, nothing is launched.
 * The index is rebuilt by every call.  sassy_hip_search with SASSY_HIP_LINE_SPANS does the same for its own matches
 * (sassy_hip_result_line_spans: one span per record, parallel to sassy_hip_result_matches; NULL without the flag);
 * sassy_hip_merge_shards does not carry spans. */
int sassy_hip_line_spans(sassy_SearcherType *s, const void *text, size_t text_len, uint32_t flags, const uint64_t *first,
                         const uint64_t *last, size_t n, sassy_hip_LineSpan *out);
uint32_t sassy_hip_line_tile(void);
/* HIP-event times (ms) of the last line-span call's index pass (count + scan) and resolve pass; timing level 2. */
int sassy_hip_line_span_times(const sassy_SearcherType *s, double *index_ms, double *resolve_ms);

/* Searcher::search_all_alignments (src/search.rs:702-760, src/alignment_iterator.rs:44-370; Python: src/python.rs:117-135):
 * every alignment of cost <= k at every end position that search_all without trace reports under this searcher's
 * settings (strands, only_best_match, the max_n_frac end-position filter).  Per end position a DFS from cell (end, m)
 * of the pattern-against-text DP matrix (top row 0, left column j) emits every path that reaches row 0 with cost <= k,
 * taking an edge ('='/'X', 'D', 'I') only if: cost so far + edge + the cell's DP value <= k; it is no leading or
 * trailing 'D'; it does not leave (by 'I'/'D') a diagonal that matches exactly up to row 0, nor enter one at a cell from
 * which the diagonal matches exactly down to the last row visited on it (row m if none; this reads text past the end
 * position); no 'I' while the indels since the last '=' are net deletions, no 'D' while they are net insertions.  The
 * surviving edges are visited by total cost, ties in the order diagonal, D, I.  The Rc strand runs on the reversed text
 * with complement(pattern), coordinates mapped back as [n - e', n - s').  Records: pattern_start 0, pattern_end m, the
 * path's own cost, the cigar as traced Rc matches carry it; with max_n_frac < 1 only alignments whose span passes.
 * Order: Fwd alignments by ascending text_end, then Rc ones by descending text_start, DFS order inside one end position
 * (a group = a maximal run of one strand and one anchor: text_end for Fwd, text_start for Rc).  Runs on the device
 * (sassy_amd/csrc/all_alignments.hip); the result is one flat sassy_hip_Result.  flags: SASSY_HIP_TEXT_ON_DEVICE,
 * SASSY_HIP_TEXT_UNCHANGED as for sassy_hip_search, anything else is SASSY_HIP_EINVAL.  Overhang searchers (alpha set):
 * SASSY_HIP_EUNSUPPORTED (the reference asserts, src/alignment_iterator.rs:61-64).  SASSY_HIP_ENOMEM (with the count in
 * the message) if the result does not fit host memory or its cigar text exceeds 4 GiB.  sassy_hip_get_stats afterwards:
 * scan_ms / filter_ms of the search, trace_ms = the HIP-event time of the enumeration launches, candidates = end
 * positions enumerated. */
int sassy_hip_search_all_alignments(sassy_SearcherType *s, const uint8_t *pattern, size_t pattern_len,
                                    const uint8_t *text, size_t text_len, size_t k, uint32_t flags,
                                    sassy_hip_Result **out);

/* Searcher::search_with_fn (src/search.rs:767-784): keep only the end positions for which the
 * callback returns non-zero.  It sees what the reference's closure sees: the pattern, the text up
 * to the end position (text_till_end[0 .. end_pos)) and the strand (0 Fwd, 1 Rc); for the Rc strand
 * both are the complemented pattern and the REVERSED text the scan ran on.  Host text only. */
typedef int (*sassy_hip_end_filter)(const uint8_t *pattern, size_t pattern_len,
                                    const uint8_t *text_till_end, size_t end_pos, int strand,
                                    void *user);
int sassy_hip_search_with_fn(sassy_SearcherType *s, const uint8_t *pattern, size_t pattern_len,
                             const uint8_t *text, size_t text_len, size_t k, uint32_t flags,
                             sassy_hip_end_filter fn, void *user, sassy_hip_Result **out);

/* Searcher::search_many / search_patterns / search_texts (src/search.rs:531-678): every pattern in
 * every text; matches carry pattern_idx and text_idx and come pattern-major (pattern 0 in text 0,
 * pattern 0 in text 1, ...), each pair in `search` order (Fwd by end position, then Rc) -- the order
 * of the reference's SearchMode::Single.  With SASSY_HIP_TEXT_ON_DEVICE the text pointers are
 * device pointers (16-byte aligned). */
int sassy_hip_search_many(sassy_SearcherType *s, const uint8_t *const *patterns,
                          const size_t *pattern_lens, size_t n_patterns, const uint8_t *const *texts,
                          const size_t *text_lens, size_t n_texts, size_t k, uint32_t flags,
                          sassy_hip_Result **out);

/* Best-cost search: the smallest cost per (pattern, text) pair, or per text the best pattern, without the records.
 * Definition (for every searcher configuration): group the matches sassy_hip_search_many returns for the same searcher,
 * inputs and k by (pattern_idx, text_idx); a pair's value is the minimum `cost` of its group.  (The report rule keeps
 * every local minimum and the global minimum of a pair is one, so without an end-position filter this is the minimum of
 * the DP's last row where it is <= k.)
 *  - strands: as the searcher (rc); Ascii with rc: SASSY_HIP_EUNSUPPORTED, as search_many;
 *  - overhang searchers (alpha, max_overhang): the cost includes the overhang price, as in the records;
 *  - max_n_frac set: only matches that pass the N filter count;
 *  - only_best_match does not change the answer (it can, together with max_n_frac: then the definition above holds);
 *  - flags: SASSY_HIP_TEXT_ON_DEVICE as for search_many, anything else SASSY_HIP_EINVAL; k > 254: SASSY_HIP_EINVAL;
 *    empty texts, k >= pattern_len, n_patterns == 0 / n_texts == 0: what search_many gives, reduced;
 *  - refused while tickets are open, like the other synchronous entry points.
 * Where search_many runs a batch of host texts in one pass (seeded search / pattern-tiled scan over the laid-out batch,
 * the per-text tiled scan of overhang searchers) the scan's (pattern, position, cost) list is reduced on the device
 * (sassy_amd/csrc/min_costs.hip): no sort, no report rule, no traceback, no records.  With max_n_frac that path needs
 * a batch of plain A C G T (the N filter cannot touch it), and best_pattern's takes fewer than 2^24 patterns;
 * everything else -- Ascii, other letters under a Dna searcher or the N filter, device-resident texts, one text,
 * patterns of several lengths -- runs
 * search_many (without trace where the N filter allows it) and reduces its records on the host.  Option
 * min_cost_device = 0: always that general path.  SASSY_HIP_ENOMEM (with the size in the message) if the device matrix
 * cannot be had.  sassy_hip_get_stats afterwards: scan_ms / filter_ms as for the search, trace_ms = the HIP-event time
 * of the reduction launches (timing level 2), candidates = list entries reduced.
 *
 * sassy_hip_min_costs: out_cost[p * n_texts + t] = that minimum over the strands searched, SASSY_HIP_NO_MATCH if there
 * is no match of cost <= k.  out_strand (may be NULL), same shape: the strand of the minimum, 0 Fwd / 1 Rc, Fwd on a
 * tie, 0 where there is no match. */
#define SASSY_HIP_NO_MATCH 255u
int sassy_hip_min_costs(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                        size_t n_patterns, const uint8_t *const *texts, const size_t *text_lens, size_t n_texts,
                        size_t k, uint32_t flags, uint8_t *out_cost, uint8_t *out_strand);
/* Per text the best pattern: out_cost[t] as above, minimised over the patterns as well; out_pattern[t] the pattern that
 * attains it (lowest index on a tie, then Fwd before Rc; UINT32_MAX where there is no match), out_strand[t] its strand.
 * out_pattern / out_strand may be NULL (a pure filter asks for out_cost only). */
int sassy_hip_best_pattern(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                           size_t n_patterns, const uint8_t *const *texts, const size_t *text_lens, size_t n_texts,
                           size_t k, uint32_t flags, uint8_t *out_cost, uint32_t *out_pattern, uint8_t *out_strand);

/* Best matches: per text the one best match over all patterns and strands, as a complete record -- where best_pattern
 * says which pattern, at what cost and on which strand, this also says where.
 * Definition (for every searcher configuration): take R = the records sassy_hip_search_many returns for the same
 * searcher with only_best_match off and default flags.  The best match of text t is the record of R with text_idx == t
 * that is smallest under this order:
 *   1. lowest cost;  2. lowest pattern_idx;  3. Fwd before Rc;
 *   4. the rightmost end in the strand's scan direction: the largest text_end for Fwd, the smallest text_start for Rc
 *      (the Rc strand is scanned on the reversed text) -- the reference's only_best_match rule, "rightmost match with
 *      minimal cost", src/search.rs:1392-1412.  (Overhang searchers: of two matches that end behind the text's end the
 *      one that hangs over further, i.e. with the smaller pattern_end, ends further right.)
 * Rules 1-3 are best_pattern's tie rule: (cost, pattern_idx, strand) of the result equal best_pattern's output text by
 * text.  A text with no match of cost <= k has no record.  The record is complete and byte for byte what search_many
 * carries for that match: text_start, text_end, pattern_start, pattern_end, cost, strand, cigar, pattern_idx, text_idx.
 * *out is an ordinary result (sassy_hip_result_free) with at most n_texts records in ascending text_idx.
 *  - flags: SASSY_HIP_TEXT_ON_DEVICE as for search_many, SASSY_HIP_WITHOUT_TRACE (end and cost only, as elsewhere: no
 *    cigar, text_start / pattern_start and the far text coordinate UINT64_MAX); anything else SASSY_HIP_EINVAL;
 *  - k > 254: SASSY_HIP_EINVAL; Ascii with rc: SASSY_HIP_EUNSUPPORTED; max_n_frac set: only matches that pass the N
 *    filter count; the searcher's only_best_match setting does not change the answer;
 *  - refused while tickets are open, like the other synchronous entry points.
 * The device path (sassy_amd/csrc/best_matches.hip) takes the call where best_pattern's device reduction does -- a batch
 * of >= 2 host texts, patterns of one length <= 64, 2k + 3 <= 64, not Ascii, fewer than 2^24 patterns, through the
 * one-pass paths -- when max_n_frac is unset, every text is shorter than 2^31 - 128 and the batch is the whole call (at
 * most 1 GiB laid out): the scan's list is reduced to one 64-bit cell per text that keeps the winning end position, one
 * candidate per text goes straight to the traceback (no sort, no report rule), and one record and cigar per text come
 * back in the pinned block the result keeps.  Everything else runs search_many and reduces its records on the host by
 * the order above; option best_match_device = 0: always that general path. */
int sassy_hip_best_matches(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                           size_t n_patterns, const uint8_t *const *texts, const size_t *text_lens, size_t n_texts,
                           size_t k, uint32_t flags, sassy_hip_Result **out);

/* Hamming search: every start s with at most k MISMATCHES -- substitutions only, no insertions or deletions -- of each
 * pattern in one text (sassy_amd/csrc/hamming.hip).  With match(p, t) the searcher's profile relation (Dna:
 * equal 2-bit codes (c >> 1) & 3; Iupac: intersecting base sets; Ascii: byte equality; ascii_ci: eq_ignore_ascii_case),
 * H(s) = #{ j < m : !match(P[j], T[s + j]) } for 0 <= s <= n - m; a hit is EVERY s with H(s) <= k (no local-minimum rule;
 * k >= m: every start; n < m: nothing).  One record per hit: text_start = s, text_end = s + m, pattern_start = 0,
 * pattern_end = m, cost = H(s), a cigar of run-length encoded '=' / 'X'.  A searcher with rc (Dna / Iupac) also searches
 * reverse_complement(P) on the forward text: those records carry strand 1 and forward-text coordinates, their cigar runs in
 * pattern direction (op j = match(complement(P[j]), T[s + m - 1 - j])), as sassy_hip_search's Rc records do.  max_n_frac
 * set: a hit is kept iff float(N in its span) / float(m) <= max_n_frac, decided on the device before the hit takes any
 * list space.  Order: (pattern_idx, Fwd before Rc, text_start) ascending -- part of the contract.
 *  - one text (a batch of texts: sassy_hip_search_hamming_many), n_patterns >= 1 patterns of any (mixed) lengths; the patterns of a launch share one pass over the text;
 *  - flags: SASSY_HIP_WITHOUT_TRACE (the same records without cigar), SASSY_HIP_TEXT_ON_DEVICE, SASSY_HIP_TEXT_UNCHANGED
 *    (accepted, nothing is cached); anything else SASSY_HIP_EINVAL;
 *  - refused before any device work: overhang searchers and only_best_match (SASSY_HIP_EUNSUPPORTED), Ascii with rc (as
 *    everywhere), an empty pattern or list, an invalid Iupac pattern, k > 0x7FFFFFFF (SASSY_HIP_EINVAL), a pattern of more
 *    than SASSY_HIP_HAMMING_MAX_ROWS rows, an Ascii pattern with more than 64 distinct (folded) bytes
 *    (SASSY_HIP_EUNSUPPORTED); Ascii pattern sets whose distinct bytes exceed 64 together are split over launches;
 *  - result limits: 2^32 records, 4 GiB of cigar text (SASSY_HIP_ENOMEM); texts of up to 2^32 - 17 blocks of 64 bytes;
 *  - sassy_hip_get_stats afterwards: scan_ms = the scan kernel's HIP-event time over all launches (timing level >= 1),
 *    scan_launches, candidates = hits, hit_blocks = 16-byte items, filtered = 7. */
#define SASSY_HIP_HAMMING_MAX_ROWS 1024
int sassy_hip_search_hamming(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                             size_t n_patterns, const void *text, size_t text_len, size_t k, uint32_t flags,
                             sassy_hip_Result **out);

/* Hamming search over a batch of texts (reads) in one call: the records are the union over t of what
 * sassy_hip_search_hamming(patterns, texts[t], k) returns for the same searcher, each with text_idx = t and coordinates
 * relative to text t; every other field is that call's (pattern_idx, cost, strand, cigar, pattern_start / pattern_end, the
 * max_n_frac rule per span).  Order: (pattern_idx, Fwd before Rc, text_idx, text_start) ascending -- part of the contract.
 * A text shorter than a pattern has no hits of it (empty texts included); n_texts == 0: an empty result, 0.
 *  - flags: SASSY_HIP_WITHOUT_TRACE (the same records without cigar); anything else, SASSY_HIP_TEXT_ON_DEVICE included,
 *    SASSY_HIP_EINVAL (host texts only);
 *  - the refusals of sassy_hip_search_hamming, with the same codes, before any device work;
 *  - the texts are laid out in one buffer, each from a multiple of 64 bytes on, in batches of at most 1 GiB (option
 *    hamming_many_batch); the scan masks every start by the bytes left in its block's own text, the emit kernel finds a
 *    hit's text in the batch's start table. */
int sassy_hip_search_hamming_many(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                                  size_t n_patterns, const uint8_t *const *texts, const size_t *text_lens, size_t n_texts,
                                  size_t k, uint32_t flags, sassy_hip_Result **out);

/* Per text the best record of sassy_hip_search_hamming_many: the smallest under (cost, pattern_idx, Fwd before Rc,
 * text_start) -- sassy_hip_best_pattern's tie rule, then the leftmost start.  out_cost[t], out_pattern[t], out_strand[t]
 * (0 Fwd / 1 Rc) and out_start[t], the start in the forward text relative to text t; a text without a hit gets
 * SASSY_HIP_NO_MATCH, UINT32_MAX, 0, UINT64_MAX.  out_pattern, out_strand and out_start may be NULL.  Demultiplexing by
 * mismatch count: which barcode, at how many mismatches, where.
 *  - no flags (host texts only): anything else SASSY_HIP_EINVAL; k > 254 SASSY_HIP_EINVAL (costs are bytes);
 *  - the refusals of sassy_hip_search_hamming; 2^23 patterns or more, or a text of 2^32 bytes or more,
 *    SASSY_HIP_EUNSUPPORTED (the device keeps cost:8 | 2 pattern_idx + strand:24 | start:32 in one 64-bit cell per text);
 *  - no records leave the device: every block's minimum goes into its text's cell, the cells come back once per batch. */
int sassy_hip_hamming_best_pattern(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                                   size_t n_patterns, const uint8_t *const *texts, const size_t *text_lens, size_t n_texts,
                                   size_t k, uint32_t flags, uint8_t *out_cost, uint32_t *out_pattern, uint8_t *out_strand,
                                   uint64_t *out_start);

/* Hamming hit counts per pattern, strand and cost, reduced on the device: out_counts[(2 p + strand) (k + 1) + c] is the
 * number of records of sassy_hip_search_hamming(patterns, text, k) with pattern_idx = p, that strand (0 Fwd / 1 Rc) and
 * cost = c, for the same searcher -- the same profile relation, rc and max_n_frac rule; the _many call counts the records of
 * sassy_hip_search_hamming_many, summed over all texts.  out_counts holds n_patterns * 2 * (k + 1) counters and is written
 * whole: the strand-1 rows of a searcher without rc are zero, and so are the bins with c > m and the rows of a pattern
 * longer than the text.  The histogram that guide and primer design ranks candidates by; no record is made.
 *  - flags: sassy_hip_hamming_counts takes SASSY_HIP_TEXT_ON_DEVICE and SASSY_HIP_TEXT_UNCHANGED (accepted, nothing is
 *    cached), sassy_hip_hamming_counts_many none (host texts only); anything else SASSY_HIP_EINVAL;
 *  - the refusals of sassy_hip_search_hamming, with the same codes, before any device work; also k > 254 (the family's
 *    byte-cost limit) and out_counts == NULL SASSY_HIP_EINVAL, a table of more than 2^32 - 1 bins SASSY_HIP_EUNSUPPORTED;
 *  - the scan kernel folds a wavefront's hits per cost into 64-bit counters, one atomic add per wavefront, pattern and cost
 *    that is present: no items, no sort, no emit kernel, no replay of a text range; one launch per pattern group takes
 *    every tile.  A small table is kept in several copies (option hamming_count_copies) that the host sums;
 *  - options hamming_batch and hamming_many_batch keep their meaning; hamming_items and hamming_records have none here;
 *  - sassy_hip_get_stats afterwards: scan_ms, scan_launches, candidates = the total of the table, filtered = 7. */
int sassy_hip_hamming_counts(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                             size_t n_patterns, const void *text, size_t text_len, size_t k, uint32_t flags,
                             uint64_t *out_counts /* n_patterns * 2 * (k + 1) */);
int sassy_hip_hamming_counts_many(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                                  size_t n_patterns, const uint8_t *const *texts, const size_t *text_lens, size_t n_texts,
                                  size_t k, uint32_t flags, uint64_t *out_counts);

/* Amplicons: which products a primer PAIR makes (in-silico PCR), joined on the device from the Hamming scan's hits.
 * With H_P(s) the mismatch count of pattern P at start s of the forward text (sassy_hip_search_hamming) and H-_P(s) that of
 * reverse_complement(P) -- what an rc searcher reports as strand 1 --, an amplicon of pair i = (F, R), both written 5'->3',
 * of lengths a and b, is (strand, start, end), L = end - start, with min_len <= L <= max_len, L >= max(a, b), and
 *   strand 0: H_F(start) <= k and H-_R(end - b) <= k;
 *   strand 1: H_R(start) <= k and H-_F(end - a) <= k (an rc searcher only).
 * EVERY such combination is a record (no nearest-partner rule); F == R or a palindromic site gives a strand-0 and a strand-1
 * record of one span, and both stay.  max_n_frac applies per primer site, as in sassy_hip_search_hamming.  A searcher
 * without rc reports strand 0 only (it still scans reverse_complement(R)).  The records are the join of what
 * sassy_hip_search_hamming({F, R}, text, k) returns on an rc searcher; order (pair_idx, strand, start, end).
 *  - flags: SASSY_HIP_TEXT_ON_DEVICE and SASSY_HIP_TEXT_UNCHANGED (accepted, nothing is cached); anything else SASSY_HIP_EINVAL;
 *  - refusals, before any device work: those of sassy_hip_search_hamming for all 2 n_pairs primers; an Ascii / ascii_ci
 *    searcher SASSY_HIP_EUNSUPPORTED (no reverse complement); k > 254, min_len == 0, min_len > max_len or
 *    max_len > SASSY_HIP_AMPLICON_MAX_LEN SASSY_HIP_EINVAL;
 *  - more than 2^32 - 1 records: SASSY_HIP_ENOMEM, the message carries the count;
 *  - *out = NULL and *n_out = 0 when there is nothing: a valid result.  A pair with a primer longer than the text has none;
 *  - options hamming_batch (scanned patterns per launch: four per pair of an rc searcher, two otherwise, a pair never
 *    split), hamming_items and hamming_records keep their meaning.  Free *out with sassy_hip_amplicons_free. */
typedef struct sassy_hip_Amplicon {
  uint64_t start, end;
  uint32_t pair_idx;
  uint8_t strand;    /* 0: F on the forward strand at start; 1: R on the forward strand at start */
  uint8_t fwd_cost;  /* the mismatches of F, whichever side it sits on */
  uint8_t rev_cost;  /* the mismatches of R */
  uint8_t pad_;      /* zero */
} sassy_hip_Amplicon;
#define SASSY_HIP_AMPLICON_MAX_LEN (1u << 24)
int sassy_hip_hamming_amplicons(sassy_SearcherType *s, const uint8_t *const *fwd, const size_t *fwd_lens,
                                const uint8_t *const *rev, const size_t *rev_lens, size_t n_pairs, const void *text,
                                size_t text_len, size_t k, uint64_t min_len, uint64_t max_len, uint32_t flags,
                                sassy_hip_Amplicon **out, size_t *n_out);
void sassy_hip_amplicons_free(sassy_hip_Amplicon *p);

/* All-vs-all Hamming distances between two lists of sequences of ONE length m, 1 <= m <= 128: there is no text, every
 * sequence of `a` meets every sequence of `b` at the one alignment there is (sassy_amd/csrc/hamming_pairs.hip; DESIGN.md
 * 5.10 "Pairs").  `a` holds n_a sequences back to back, m bytes each, as sassy_hip_encode_patterns takes its patterns; so
 * does `b`.  With match() the searcher's profile relation exactly as sassy_hip_search_hamming defines it,
 *   H(x, y)  = #{ t < m : !match(x[t], y[t]) }   (strand 0),
 *   H-(x, y) = H(x, reverse_complement(y))       (strand 1, an rc searcher only).
 * Two-set mode: a pair is every (i, j, strand) with cost <= k, 0 <= i < n_a, 0 <= j < n_b.  Self mode (b == NULL and
 * n_b == 0): b = a and every unordered pair once -- strand 0: i < j only; strand 1: i <= j (H- is symmetric in i and j);
 * (i, i, 1) stays: a sequence within k of its own reverse complement is a real collision.  Barcode / UMI / guide set design,
 * whitelist correction, collisions between two panels.
 *  - sassy_hip_hamming_pairs: every pair as a record, in ascending (a_idx, b_idx, strand) order -- part of the contract;
 *    *out = NULL and *n_out = 0 when there is none: a valid result; more than 2^32 - 1 records: SASSY_HIP_ENOMEM, the
 *    message carries the count.  Free *out with sassy_hip_hamming_pairs_free.
 *  - sassy_hip_hamming_nearest: per a_i the smallest candidate (j, strand), cost <= k, under (cost, b_idx, Fwd before Rc) --
 *    the tie rule of sassy_hip_best_pattern and sassy_hip_hamming_best_pattern; out_ties[i] = the candidates at that cost
 *    (a correction is unambiguous iff it is 1).  Self mode: the full square, only (j == i, strand 0) is no candidate.  An
 *    entry without a candidate gets SASSY_HIP_NO_MATCH, UINT32_MAX, 0, 0.  out_index, out_strand and out_ties may be NULL.
 *  - flags: none (the sequences are host bytes): anything else SASSY_HIP_EINVAL;
 *  - refusals, before any device work: m == 0, m > 128, k > 254, n_a == 0, a non-NULL b with n_b == 0, a NULL b with
 *    n_b > 0 and NULL out pointers SASSY_HIP_EINVAL; n_a or n_b > 2^31 - 1 and a searcher with max_n_frac (there is no
 *    text span for it to apply to) SASSY_HIP_EUNSUPPORTED; then those of sassy_hip_search_hamming for each list as they stand,
 *    a first, the message followed by "(<entry point>: list a)" or "(... list b)" and its "pattern N" counting inside that
 *    list.  This includes the family's Ascii limit -- an ascii / ascii_ci sequence of more than 64 distinct (folded) bytes is
 *    SASSY_HIP_EUNSUPPORTED -- which the bit planes here would not need: kept so that the family refuses one set of inputs;
 *  - a host table or plane array that cannot be allocated: SASSY_HIP_ENOMEM (nothing throws across the C boundary);
 *  - the host encodes the sequences into bit planes (Dna 2, Iupac 4, Ascii 8; ascii_ci folded first) and the reverse
 *    complements of b as target records of their own; a lane owns one entry of a and walks the targets of its chunk, the
 *    grid is strips of 256 entries x chunks of targets (option pairs_chunks: geometry only).  A survey pass leaves one cell
 *    per entry and chunk; _nearest folds them in chunk order; _pairs scans the counts and a fill pass writes the records in
 *    place -- no sort, no atomic;
 *  - sassy_hip_get_stats afterwards: filtered = 8, chunks, grid = strips, candidates = the records (_pairs); at timing
 *    level 2 filter_ms = the survey, trace_ms = the fill, scan_ms = all device passes. */
typedef struct sassy_hip_HammingPair {
  uint32_t a_idx, b_idx;
  uint8_t cost;
  uint8_t strand;   /* 0: H(a, b); 1: H(a, reverse_complement(b)) */
  uint8_t pad_[2];  /* zero */
} sassy_hip_HammingPair; /* 12 bytes */
int sassy_hip_hamming_pairs(sassy_SearcherType *s, const uint8_t *a, size_t n_a, const uint8_t *b, size_t n_b, size_t m,
                            size_t k, uint32_t flags, sassy_hip_HammingPair **out, size_t *n_out);
void sassy_hip_hamming_pairs_free(sassy_hip_HammingPair *p);
int sassy_hip_hamming_nearest(sassy_SearcherType *s, const uint8_t *a, size_t n_a, const uint8_t *b, size_t n_b, size_t m,
                              size_t k, uint32_t flags, uint8_t *out_cost, uint32_t *out_index, uint8_t *out_strand,
                              uint32_t *out_ties);

/* All-vs-all edit distances between two lists of sequences: sassy_hip_hamming_pairs / _nearest with the Levenshtein distance
 * in place of H, so that a sequence that lost or gained a base is near its origin (sassy_amd/csrc/edit_pairs.hip; DESIGN.md
 * 5.10 "Edit pairs").  `a` holds n_a sequences of m_a bytes back to back, `b` holds n_b sequences of m_b bytes,
 * 1 <= m_a, m_b <= 64; the two lengths may differ.  With match() the searcher's profile relation exactly as
 * sassy_hip_search_hamming defines it,
 *   E(x, y)  = the fewest substitutions, insertions and deletions (1 each) that turn x into y under match(): both
 *              sequences are consumed whole, D[0][j] = j and D[i][0] = i                         (strand 0),
 *   E-(x, y) = E(x, reverse_complement(y))                                                       (strand 1, an rc searcher only).
 * Everything else is the Hamming pair calls' contract word for word: two-set mode and self mode (b == NULL and n_b == 0;
 * m_b is then 0 or m_a), the self-mode triangle -- strand 0: i < j, strand 1: i <= j, (i, i, 1) stays --, records in
 * ascending (a_idx, b_idx, strand) order, _nearest under (cost, b_idx, Fwd before Rc) with out_ties over the full square
 * without (i, i, 0) in self mode, SASSY_HIP_NO_MATCH, UINT32_MAX, 0, 0 for an entry without a candidate, *out = NULL and
 * *n_out = 0 for no record, more than 2^32 - 1 records SASSY_HIP_ENOMEM with the count.  Free *out with
 * sassy_hip_edit_pairs_free.  out_index, out_strand and out_ties may be NULL.
 *  - flags: none: anything else SASSY_HIP_EINVAL;
 *  - refusals, before any device work: m_a or m_b == 0 or > 64, k > 254, n_a == 0, a non-NULL b with n_b == 0, a NULL b
 *    with n_b > 0, a NULL b with m_b neither 0 nor m_a and NULL out pointers SASSY_HIP_EINVAL; n_a or n_b > 2^31 - 1 and a
 *    searcher with max_n_frac SASSY_HIP_EUNSUPPORTED; then those of sassy_hip_search_hamming for each list as they stand,
 *    named as the Hamming pair calls name them ("(<entry point>: list a)");
 *  - |m_a - m_b| > k is a valid call with an empty answer (E >= |m_a - m_b|): the device is acquired -- a machine without
 *    one still fails -- and nothing is launched;
 *  - a host table that cannot be allocated: SASSY_HIP_ENOMEM;
 *  - the host encodes the entries of a into the bit planes of the Hamming pair calls and the targets into one row code per
 *    column; a lane owns one entry and steps a bit-vector column (Myers / Hyyro, global boundary) per target column, several
 *    targets side by side; grid, survey, scan and fill are those of sassy_hip_hamming_pairs (option pairs_chunks: geometry
 *    only);
 *  - sassy_hip_get_stats afterwards: filtered = 9, chunks, grid = strips, candidates = the records (_pairs); at timing
 *    level 2 filter_ms = the survey, trace_ms = the fill, scan_ms = all device passes. */
typedef sassy_hip_HammingPair sassy_hip_EditPair; /* the same 12 bytes; cost = E */
int sassy_hip_edit_pairs(sassy_SearcherType *s, const uint8_t *a, size_t n_a, size_t m_a, const uint8_t *b, size_t n_b,
                         size_t m_b, size_t k, uint32_t flags, sassy_hip_EditPair **out, size_t *n_out);
void sassy_hip_edit_pairs_free(sassy_hip_EditPair *p);
int sassy_hip_edit_nearest(sassy_SearcherType *s, const uint8_t *a, size_t n_a, size_t m_a, const uint8_t *b, size_t n_b,
                           size_t m_b, size_t k, uint32_t flags, uint8_t *out_cost, uint32_t *out_index, uint8_t *out_strand,
                           uint32_t *out_ties);

/* Sequence clustering (sassy_amd/csrc/clusters.hip; DESIGN.md 5.10 "Clusters"): the connected components of the within-k
 * graph of ONE list -- UMI deduplication, collapsing barcodes onto their origins, collision groups of a panel -- without
 * the pair records.  a: n sequences of m bytes each, laid out as the pair calls take them; m <= 128 (_hamming_) or <= 64
 * (_edit_).  The graph has an edge {i, j}, i != j, where H(a_i, a_j) <= k (E(a_i, a_j) <= k) under the family's relation
 * and, for an rc searcher, also where the distance of a_i to reverse_complement(a_j) is <= k: exactly the records (i, j,
 * strand) of the self-mode pair call, (i, i, 1) left out.  The Iupac relation is not transitive (N meets everything);
 * components are well defined all the same.
 *  - out_label[i] (n entries, required): the SMALLEST index of i's connected component -- one fixed array, whatever the
 *    device's schedule; out_size[i] (n entries, may be NULL): the size of that component; *n_clusters (may be NULL): the
 *    number of i with out_label[i] == i;
 *  - refused before any device work, as the self-mode pair call of the same distance refuses: NULL s, a or out_label, any
 *    flag, m == 0, m over the limit, k > 254, n == 0 (SASSY_HIP_EINVAL); n > 2^31 - 1, a searcher with max_n_frac, and what
 *    the Hamming family refuses (SASSY_HIP_EUNSUPPORTED / _EINVAL); k >= m: one cluster;
 *  - the device walks the self-mode triangle of the pair call once (option pairs_chunks: geometry only) and joins the two
 *    trees of every candidate pair in one array of n indices, lock-free (parent[x] <= x, roots linked larger under smaller
 *    by compare-and-swap); no cell matrix, no scan, no fill, no record.  Device memory: the encoded list and 8 n bytes;
 *  - sassy_hip_get_stats afterwards: filtered = 10 (_hamming_) or 11 (_edit_), chunks, grid = strips, text_bytes; at timing
 *    level 2 filter_ms = the link pass, scan_ms = link + flatten. */
int sassy_hip_hamming_clusters(sassy_SearcherType *s, const uint8_t *a, size_t n, size_t m, size_t k, uint32_t flags,
                               uint32_t *out_label, uint32_t *out_size, size_t *n_clusters);
int sassy_hip_edit_clusters(sassy_SearcherType *s, const uint8_t *a, size_t n, size_t m, size_t k, uint32_t flags,
                            uint32_t *out_label, uint32_t *out_size, size_t *n_clusters);

/* UMI grouping (sassy_amd/csrc/umi_groups.hip; DESIGN.md 5.10 "UMI groups"): identical reads counted and collapsed, the
 * distinct sequences compared with each other only, and an abundant sequence absorbing its rare neighbours -- UMI-tools'
 * `directional` method with the tie order fixed.  a, n, m as sassy_hip_hamming_clusters takes them (m <= 128); Hamming only.
 *  - duplicates: two sequences whose bit planes (the pair family's encoding) are equal.  Dna: the planes hold (c >> 1) & 3 per
 *    row, so upper and lower case fold and so do all bytes that share that code (A / a, C / c, T / t / U / u, G / g -- and N
 *    with G's code: Dna has no N of its own).  Iupac: the planes hold the letter's set of bases, so case folds and letters
 *    with one set are one (T / U); N and A MATCH but are no duplicates.  Ascii: the byte itself, nothing folds; ascii_ci: the
 *    folded byte, A-Z onto a-z only.  out_rep[i] (may be NULL): the smallest j that is a duplicate of i -- out_rep[i] == i
 *    marks the distinct sequences; out_count[i] (may be NULL): the duplicates of i, itself included; *n_unique (may be NULL):
 *    the number of i with out_rep[i] == i;
 *  - groups are formed over the distinct sequences, each named by its first index u and carrying its count c_u.  u and v are
 *    neighbours where the self-mode pair call on the distinct sequences has a record (u, v, strand), u != v -- H <= k on
 *    either strand for an rc searcher; (u, u, 1) is no edge.  SASSY_HIP_UMI_UNIQUE: label = rep, k is ignored.
 *    SASSY_HIP_UMI_CLUSTER: the connected components; out_label and out_size are exactly sassy_hip_hamming_clusters' on the
 *    full list.  SASSY_HIP_UMI_DIRECTIONAL: an edge u -> v where u and v are neighbours and c_u >= 2 c_v - 1 (two sequences of
 *    count 1 point at each other); the distinct sequences ordered by (count descending, first index ascending) and gone
 *    through in that order, one that is in no group yet opens a group and takes every sequence reachable from it along edges
 *    that is in no group yet; the label of v is the opener of its group -- the first in the order among all u from which v
 *    is reachable, v included;
 *  - out_label[i] (n entries, required): the label of out_rep[i], an index into a; out_size[i] (may be NULL): the READS, not
 *    the distinct sequences, that share that label; *n_groups (may be NULL): the number of i with out_label[i] == i.  The
 *    arrays are the same on every run, whatever the device's schedule and whatever the table's hash;
 *  - refused before any device work: what sassy_hip_hamming_clusters refuses, by the same function; an unknown method
 *    SASSY_HIP_EINVAL.  More than 2^32 - 1 pair records among the distinct sequences (DIRECTIONAL): SASSY_HIP_ENOMEM with
 *    the count, as the pair call fails, once the survey has counted them.  k >= m is cut to m;
 *  - the device: an open-addressing table of 32-bit slots keyed by a hash of the plane words (option collapse_slots:
 *    geometry only), a scan of the flags rep[i] == i for the distinct sequences' numbering, a gather of their planes, the pair
 *    call's passes over those (CLUSTER: its link pass; DIRECTIONAL: survey, scan, fill -- the records stay on the device),
 *    DIRECTIONAL: a relaxation of 64-bit labels over the records, launched until nothing falls (at most n_unique + 1
 *    launches), then one pass per distinct sequence for the groups' sizes and one per read for the columns;
 *  - sassy_hip_get_stats afterwards: filtered = 12, candidates = the records among the distinct sequences (DIRECTIONAL; else
 *    0), chunks, grid = strips of that walk, hit_blocks = n_unique, blocks = the relaxation's launches; at timing level 2
 *    (the events ev_line[0 .. 3] of the searcher) filter_ms = the walk passes over the distinct sequences ([1] -> [2]),
 *    trace_ms = the relaxation (CLUSTER: the flatten) with the size and expand passes ([2] -> [3]), scan_ms = those and the
 *    collapse -- table, lookup, scan, gather ([0] -> [1]) --, so the collapse alone is scan_ms - filter_ms - trace_ms. */
#define SASSY_HIP_UMI_UNIQUE      0u  /* collapse only: a group is a set of identical sequences; k is ignored */
#define SASSY_HIP_UMI_CLUSTER     1u  /* connected components within k, on the distinct sequences */
#define SASSY_HIP_UMI_DIRECTIONAL 2u  /* the count-aware rule above */
int sassy_hip_umi_groups(sassy_SearcherType *s, const uint8_t *a, size_t n, size_t m, size_t k,
                         uint32_t method, uint32_t flags,
                         uint32_t *out_label, uint32_t *out_size,   /* n entries; out_size may be NULL */
                         uint32_t *out_rep, uint32_t *out_count,    /* n entries; either may be NULL */
                         size_t *n_unique, size_t *n_groups);       /* may be NULL */

/* FASTA unwrap on the device (sassy_amd/csrc/fasta_unwrap.hip): the raw bytes of a chunk of FASTA in, every
 * record's sequence out as a device-resident text that the one-text entry points take with SASSY_HIP_TEXT_ON_DEVICE, plus a
 * small host table.  `raw` holds n bytes, is empty or begins with '>', and holds whole records.  The definition is the
 * line-by-line parse: split at '\n' (a final empty piece is no line), strip one trailing '\r' from each line; a line that begins
 * with '>' opens a record whose id is the rest of that line; every other line is appended to the open record's sequence.
 * Nothing else is touched (case, N, a '>' that does not begin a line, a '\r' elsewhere).
 *  - the text: one device buffer of sassy_hip_fasta_text_bytes bytes; record r's sequence lies at [seq_start, seq_start +
 *    seq_len), seq_start a multiple of 64; the bytes between the sequences are 0 and 64 zero bytes follow the last one (they
 *    are counted in text_bytes); an empty record takes no block and shares its start with the next record;
 *  - the table: one sassy_hip_FastaRecord per record in file order; id_start / id_len index `raw` (the id without '>' and
 *    without the line's trailing '\r'), seq_start / seq_len the text;
 *  - flags: SASSY_HIP_TEXT_ON_DEVICE: `raw` is a device pointer, 16-byte aligned and readable up to the next multiple of 64
 *    behind n; 0: host bytes, uploaded once.  Takes no searcher: it runs on the calling thread's current device, on
 *    `hip_stream` (NULL: the default stream), and returns when the table is on the host;
 *  - refused before any device work: null arguments with n > 0, an unknown flag bit, a device pointer that is not 16-byte
 *    aligned, a first byte that is not '>' (SASSY_HIP_EINVAL; a device-resident first byte is read back first); more than
 *    2^31 - 1 super-tiles of 64 KiB, i.e. n > 2^47 - 65536 (SASSY_HIP_EUNSUPPORTED); no device SASSY_HIP_ENODEVICE.  More
 *    than 2^32 - 1 records is SASSY_HIP_EUNSUPPORTED as well, known once the count pass has run.
 * The handle owns the text: sassy_hip_fasta_free releases it (the text of every record with it). */
typedef struct sassy_hip_FastaRecord {
  uint64_t id_start, id_len;   /* in the raw bytes */
  uint64_t seq_start, seq_len; /* in the device text */
} sassy_hip_FastaRecord;
typedef struct sassy_hip_Fasta sassy_hip_Fasta;
int sassy_hip_fasta_unwrap(const void *raw, uint64_t n, uint32_t flags, void *hip_stream, sassy_hip_Fasta **out);
uint64_t sassy_hip_fasta_n_records(const sassy_hip_Fasta *f);
const sassy_hip_FastaRecord *sassy_hip_fasta_records(const sassy_hip_Fasta *f); /* NULL without records */
void *sassy_hip_fasta_text(const sassy_hip_Fasta *f);                           /* the device pointer */
uint64_t sassy_hip_fasta_text_bytes(const sassy_hip_Fasta *f);
void sassy_hip_fasta_free(sassy_hip_Fasta *f);

/* FASTQ parse on the device (sassy_amd/csrc/fastq_reads.hip): the raw bytes of a chunk of FASTQ in, a read
 * batch out that stays on the device in the layout the Hamming batch kernels scan, plus a small host table.  `raw` holds n
 * bytes, is empty or begins with '@', and holds whole records.  The definition is strict four-line FASTQ: split at '\n' (a
 * final empty piece is no line), strip one trailing '\r' from each line; with L lines, record r is lines 4r .. 4r + 3: line 4r
 * begins with '@' and the id is the rest of it, line 4r + 1 is the sequence, line 4r + 2 begins with '+' and its content is
 * ignored, line 4r + 3 is the quality, whose length is reported and not compared.  Nothing else is touched (case, N, an '@'
 * or '+' that opens a quality line, a '\r' elsewhere).  Empty input is valid: 0 records.
 *  - malformed input is SASSY_HIP_EINVAL, and the message names the smallest malformed record and the rule it breaks: a
 *    line 4r without its '@', a line 4r + 2 without its '+', or, where L is no multiple of 4, the last record (index L / 4),
 *    which lacks lines.  Multi-line FASTQ is malformed input;
 *  - the text: one device buffer of sassy_hip_reads_text_bytes bytes; read r's sequence lies at [seq_start, seq_start +
 *    seq_len), seq_start a multiple of 64; the bytes between the sequences are 0 and 64 zero bytes follow the last one (they
 *    are counted in text_bytes); an empty sequence takes no block and shares its start with the next read, trailing empty
 *    reads start at the layout's size (text_bytes - 64);
 *  - the table: one sassy_hip_ReadRecord per record in file order; id_start / id_len (the id without '@' and without the
 *    line's trailing '\r') and qual_start / qual_len index `raw`, seq_start / seq_len the text; sassy_hip_reads_longest is
 *    the longest seq_len;
 *  - flags: SASSY_HIP_TEXT_ON_DEVICE: `raw` is a device pointer, 16-byte aligned and readable up to the next multiple of 64
 *    behind n; 0: host bytes, uploaded once.  Takes no searcher: it runs on the calling thread's current device, on
 *    `hip_stream` (NULL: the default stream), and returns when the table is on the host.  SASSY_HIP_KEEP_QUALITY: the handle
 *    also owns a quality buffer of text_bytes bytes in the layout of the text (sassy_hip_reads_quality): the quality of read
 *    r lies at [seq_start, seq_start + seq_len), the pads and the 64 spare bytes are 0.  Only under this flag a record whose
 *    quality is not as long as its sequence is SASSY_HIP_EINVAL (the message names the smallest such record; a file that is
 *    malformed as well gets the verdict above).  Without the flag nothing is kept and sassy_hip_reads_quality is NULL;
 *  - refused before any device work: null arguments with n > 0, an unknown flag bit, a device pointer that is not 16-byte
 *    aligned, a first byte that is not '@' (SASSY_HIP_EINVAL; a device-resident first byte is read back first); more than
 *    2^31 - 1 super-tiles of 64 KiB, i.e. n > 2^47 - 65536 (SASSY_HIP_EUNSUPPORTED); no device SASSY_HIP_ENODEVICE.  More
 *    than 2^32 - 1 records is SASSY_HIP_EUNSUPPORTED as well, known once the count pass has run.
 * The handle owns the text, the device copies of the starts and the lengths (uint64 each, n starts, then n lengths), the
 * table of the bytes left in its own read per 64-byte block of the text (uint32; sassy_hip_reads_rem is its device pointer,
 * (text_bytes - 64) / 64 entries) and the number of the device it was made on: sassy_hip_reads_free releases all of it. */
typedef struct sassy_hip_ReadRecord {
  uint64_t id_start, id_len;     /* in raw: the id without '@' and without the '\r' */
  uint64_t seq_start, seq_len;   /* in the device text; seq_start a multiple of 64 */
  uint64_t qual_start, qual_len; /* in raw; in a handle made by sassy_hip_merge_pairs: in the handle's own quality buffer
                                    (qual_start == seq_start), and id_start == id_len == 0 there */
} sassy_hip_ReadRecord;
typedef struct sassy_hip_Reads sassy_hip_Reads;
int sassy_hip_fastq_parse(const void *raw, uint64_t n, uint32_t flags, void *hip_stream, sassy_hip_Reads **out);
uint64_t sassy_hip_reads_n(const sassy_hip_Reads *r);
const sassy_hip_ReadRecord *sassy_hip_reads_records(const sassy_hip_Reads *r); /* NULL without records */
void *sassy_hip_reads_text(const sassy_hip_Reads *r);                          /* the device pointer */
uint64_t sassy_hip_reads_text_bytes(const sassy_hip_Reads *r);
uint64_t sassy_hip_reads_longest(const sassy_hip_Reads *r);
const uint32_t *sassy_hip_reads_rem(const sassy_hip_Reads *r); /* the device pointer */
const uint8_t *sassy_hip_reads_quality(const sassy_hip_Reads *r); /* the device pointer; NULL where qualities were not kept */
void sassy_hip_reads_free(sassy_hip_Reads *r);

/* The Hamming batch calls over a resident read batch: each returns exactly what its _many sibling (sassy_hip_search_hamming_many,
 * sassy_hip_hamming_best_pattern, sassy_hip_hamming_counts_many) returns for the host list of the handle's sequences in file
 * order -- fields, order, tie rule and limits are the sibling's -- with `reads` in the place of texts, text_lens, n_texts.
 *  - the sibling's refusals, with the same codes, before any device work (a read of 2^32 bytes or more for best_pattern);
 *    reads == NULL SASSY_HIP_EINVAL; a handle made on another device than the searcher's SASSY_HIP_EINVAL;
 *  - flags: sassy_hip_search_hamming_reads takes SASSY_HIP_WITHOUT_TRACE, the other two none; anything else SASSY_HIP_EINVAL;
 *  - the handle is scanned whole, as one batch whose first text has index 0: no upload, no layout and no table is built in
 *    these calls, and option hamming_many_batch has no meaning here; hamming_batch, hamming_items, hamming_records and
 *    hamming_count_copies keep theirs;
 *  - the handle is only read: it serves any number of calls, of any searcher on its device, one call at a time. */
int sassy_hip_search_hamming_reads(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                                   size_t n_patterns, const sassy_hip_Reads *reads, size_t k, uint32_t flags,
                                   sassy_hip_Result **out);
int sassy_hip_hamming_best_pattern_reads(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                                         size_t n_patterns, const sassy_hip_Reads *reads, size_t k, uint32_t flags,
                                         uint8_t *out_cost, uint32_t *out_pattern, uint8_t *out_strand, uint64_t *out_start);
int sassy_hip_hamming_counts_reads(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                                   size_t n_patterns, const sassy_hip_Reads *reads, size_t k, uint32_t flags,
                                   uint64_t *out_counts /* n_patterns * 2 * (k + 1) */);

/* The edit-distance batch calls over a resident read batch: each returns exactly what its sibling
 * (sassy_hip_search_many, sassy_hip_min_costs, sassy_hip_best_pattern, sassy_hip_best_matches) returns for the host list of
 * the handle's sequences in file order -- fields, order, tie rules, limits and refusals are the sibling's -- with `reads` in
 * the place of texts, text_lens, n_texts.
 *  - where the sibling lays a batch of host texts out on the host and uploads it (its one-pass paths), a kernel lays the
 *    resident reads out into the same buffer, byte for byte the same (sassy_hip_reads_relayout): no host layout, no upload;
 *    everything behind the layout is the sibling's code.  A Dna searcher's "plain A, C, G, T only" look at the texts is made
 *    on the device, over the sequences alone (the zeros between them do not count);
 *  - where the one-pass paths decline (fewer than 2 reads, a Dna batch with other letters that the per-text path does not
 *    take either, patterns of mixed lengths on a filterable shape, 2^24 reads or more, ...) the call runs the sibling's
 *    general path on the reads where they lie, as device texts;
 *  - additional refusals: reads == NULL SASSY_HIP_EINVAL; a handle made on another device than the searcher's
 *    SASSY_HIP_EINVAL; SASSY_HIP_TEXT_ON_DEVICE in flags SASSY_HIP_EINVAL (it has no meaning here); searches in flight on
 *    the searcher are refused as elsewhere;
 *  - the handle is only read: it serves any number of calls, the Hamming ones included, one call at a time. */
int sassy_hip_search_many_reads(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                                size_t n_patterns, const sassy_hip_Reads *reads, size_t k, uint32_t flags,
                                sassy_hip_Result **out);
int sassy_hip_min_costs_reads(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                              size_t n_patterns, const sassy_hip_Reads *reads, size_t k, uint32_t flags, uint8_t *out_cost,
                              uint8_t *out_strand);
int sassy_hip_best_pattern_reads(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                                 size_t n_patterns, const sassy_hip_Reads *reads, size_t k, uint32_t flags, uint8_t *out_cost,
                                 uint32_t *out_pattern, uint8_t *out_strand);
int sassy_hip_best_matches_reads(sassy_SearcherType *s, const uint8_t *const *patterns, const size_t *pattern_lens,
                                 size_t n_patterns, const sassy_hip_Reads *reads, size_t k, uint32_t flags,
                                 sassy_hip_Result **out);
/* The relayout itself, for a host that builds a batch of its own: reads first .. first + count of the handle into d_dst (device
 * memory of at least `total` bytes, 16-byte aligned), read first + i at [dst_starts[i], dst_starts[i] + seq_len) -- dst_starts
 * is a host table, ascending, no read over the next one's start or over `total` --, every other byte of [0, total) = pad;
 * bytes behind `total` are not written.  Runs on the handle's device, on hip_stream (NULL: the default stream), and returns
 * when the buffer is written.  Null arguments, a range outside the handle, a destination that is not 16-byte aligned and a
 * table the reads do not fit are SASSY_HIP_EINVAL. */
int sassy_hip_reads_relayout(const sassy_hip_Reads *reads, uint64_t first, uint64_t count, const uint64_t *dst_starts,
                             uint64_t total, uint8_t pad, void *d_dst, void *hip_stream);

/* Paired-end read overlap (sassy_amd/csrc/read_overlaps.hip, arithmetic in overlap_step.h): the best overlap
 * of the two reads of every pair, both read batches resident on the device.  The definition is
 * tests/helpers/read_overlaps_ref.py.  Pair r: a = read r of r1 (la bytes), b = the reverse complement of read r of r2 (lb
 * bytes; the profile's complement, byte by byte).  The offset d, -(lb - 1) <= d <= la - 1, places b[0] under a[d]:
 * lo = max(0, d), hi = min(la, d + lb), the overlap is ov = hi - lo rows and
 *   mm(d) = #{ i in [lo, hi) : !match(a[i], b[i - d]) },   match: the searcher's profile relation, a on the pattern side.
 *  - an offset is ACCEPTED when ov >= min_overlap, mm <= k and mm * 1000 <= max_permille * ov (integers, no floats);
 *  - the BEST accepted offset is the one of the lowest mismatch density (mm1 * ov2 < mm2 * ov1), at equal density of the
 *    larger ov, at equal ov of the larger d (FLASH's rule with the ties fixed: a non-read-through alignment beats its mirror
 *    image); the order is total, so the record is the same on every run;
 *  - out[r], 16 bytes: the best offset, its overlap and mismatches, and n_accepted, the number of accepted offsets (above 1:
 *    repeats, low-complexity reads).  No accepted offset, or an empty read on either side: all four fields zero;
 *  - derived on the host: d >= 0: insert = max(la, d + lb), both reads are kept whole; d < 0 (read-through: the insert is
 *    shorter than the reads and their tails are adapter): insert = ov, keep min(la, d + lb) bytes of read 1 and lb + d of
 *    read 2; no overlap: insert 0 (Python: sassy_amd.overlap_trims);
 *  - Iupac: R2's bytes are complemented as the reference's profile does it (U is its own complement and matches as T; what
 *    is no letter stays as it is and matches as N; X matches nothing).  Dna: both batches must hold A, C, G, T only (looked
 *    at on the device once per call and handle, in either case, as the _reads calls look; a lower-case letter keeps its
 *    2-bit code and, as in the reference's profile, is not complemented) -- anything else is SASSY_HIP_EINVAL and the message
 *    points to an iupac searcher: the 2-bit codes would let N match G, and N has no complement there;
 *  - k is not capped at 254: mismatches are 32-bit here; k beyond the longest read accepts what k = 512 accepts;
 *  - refused before any device work, SASSY_HIP_EINVAL unless noted: s == NULL; any flag; min_overlap == 0;
 *    max_permille > 1000; an Ascii searcher (no complement); overhang, only_best_match, max_n_frac set
 *    (SASSY_HIP_EUNSUPPORTED, as the Hamming family refuses them); r1 or r2 NULL; different record counts; a handle made on
 *    another device than the searcher's; a read longer than SASSY_HIP_OVERLAP_MAX_LEN in either handle (such a pair is never
 *    launched); out == NULL with pairs to write; searches in flight on the searcher.  Zero pairs: success, nothing written;
 *  - both handles are only read.  One launch, one wavefront per pair; option-free. */
#define SASSY_HIP_OVERLAP_MAX_LEN 512u
typedef struct sassy_hip_ReadOverlap {
  int32_t offset;      /* d of the best accepted offset */
  uint32_t overlap;    /* its ov */
  uint32_t mismatches; /* its mm */
  uint32_t n_accepted; /* accepted offsets of the pair; 0: no overlap, every field is 0 */
} sassy_hip_ReadOverlap;
int sassy_hip_read_overlaps(sassy_SearcherType *s, const sassy_hip_Reads *r1, const sassy_hip_Reads *r2, uint32_t min_overlap,
                            size_t k, uint32_t max_permille, uint32_t flags, sassy_hip_ReadOverlap *out /* sassy_hip_reads_n(r1) */);

/* Paired-end merge (sassy_amd/csrc/merge_pairs.hip, arithmetic in merge_step.h): every pair with an accepted
 * overlap becomes one merged read with consensus sequence and consensus quality, in a NEW read batch resident on the device
 * that every _reads entry point takes.  The definition is tests/helpers/merge_pairs_ref.py.  Pair r: a = read r of r1 with
 * qualities qa, b = the reverse complement of read r of r2 with r2's qualities reversed, qb; (d, ov, mm, n_accepted) = the
 * pair's sassy_hip_read_overlaps record under min_overlap, k, max_permille.
 *  - n_accepted == 0 (an empty read included): the pair is not merged, its merged read is empty;
 *  - otherwise the merged read has L = max(la, d + lb) columns for d >= 0 and L = ov for d < 0 (read-through: r2's head and
 *    r1's tail beyond the overlap are adapter and are dropped).  Column p is row p of a where p < la and row p - d of b where
 *    0 <= p - d < lb;
 *  - a column that one read covers takes its byte and quality; where both cover it and the bytes are equal (as bytes), that
 *    byte with the higher quality; where they differ -- whether or not the profile's relation calls them a match --, the byte
 *    of the higher quality, a's on a tie, with quality min(126, 33 + max(2, |qa - qb|)) (FLASH's rule with the tie fixed).  No
 *    quality byte is validated;
 *  - *out_merged: an ordinary sassy_hip_Reads on the searcher's device with qualities kept, ONE RECORD PER PAIR: record r is
 *    empty iff pair r was not merged.  id_start = id_len = 0 (the ids are r1's), qual_start = seq_start and qual_len = seq_len
 *    index the handle's own quality buffer.  Zero pairs, or no pair merged: text_bytes == 64.  The caller frees it with
 *    sassy_hip_reads_free;
 *  - out_overlaps, where given, receives exactly what sassy_hip_read_overlaps writes (sassy_hip_reads_n(r1) records);
 *  - refused before any device work, in this order: everything sassy_hip_read_overlaps refuses, with its codes (out_overlaps
 *    may be NULL); a handle that was parsed without SASSY_HIP_KEEP_QUALITY (SASSY_HIP_EINVAL); out_merged == NULL
 *    (SASSY_HIP_EINVAL).  A Dna batch with other bytes than A, C, G, T is refused as there.  *out_merged is NULL after every
 *    refusal;
 *  - both input handles are only read.  Device work on the searcher's stream: the overlap kernel, the layout scan of the
 *    parse over the merged lengths, one host wait for the layout's size, one write kernel indexed by 64-byte block of the
 *    output.  Stats as sassy_hip_read_overlaps leaves them, with candidates = the number of merged pairs and scan_launches = 5
 *    (the overlap kernel, the three kernels of the layout scan, the write kernel; the Dna look is not counted, as there).  Zero
 *    pairs launch no kernel: scan_launches = 0. */
int sassy_hip_merge_pairs(sassy_SearcherType *s, const sassy_hip_Reads *r1, const sassy_hip_Reads *r2, uint32_t min_overlap,
                          size_t k, uint32_t max_permille, uint32_t flags,
                          sassy_hip_ReadOverlap *out_overlaps /* may be NULL; sassy_hip_reads_n(r1) */,
                          sassy_hip_Reads **out_merged);

/* Adapter and quality trimming (sassy_amd/csrc/trim_reads.hip, arithmetic in trim_step.h): the 3' adapter and
 * the low-quality tail cut off every read of a resident batch, what is left too short dropped, in a NEW read batch resident on
 * the device that every _reads entry point, sassy_hip_merge_pairs and another trim take.  The definition is
 * tests/helpers/trim_reads_ref.py.  Read a of la bytes with qualities q; adapters p_0 .. p_{A-1}, p_j of m_j bytes, written
 * 5'->3' as they appear behind the insert.  Integers only, no floats.
 *  - QUALITY (the BWA / cutadapt 3' rule, Phred+33 fixed): quality_cutoff == 0: lq = la.  Otherwise walk i = la - 1 .. 0 with
 *    s += q[i] - 33 - quality_cutoff (signed), stop at the first i where s > 0; lq is the i of the strictly smallest s seen
 *    before the stop (s < min, min starting at 0), la where no s was below 0;
 *  - ADAPTER, on a[0:lq]: position c places p_j[0] under a[c]; ov = min(m_j, lq - c);
 *      mm(c, j) = #{ i < ov : !match(p_j[i], a[c + i]) },   match: the searcher's profile relation, the adapter on the
 *    pattern side (under Iupac an N in an adapter is a wildcard).  A position is ACCEPTED when ov >= min_overlap, mm <= k and
 *    mm * 1000 <= max_permille * ov (sassy_hip_read_overlaps' rule).  The BEST accepted position: the smallest c (the
 *    leftmost removes the most: fastp's and Trimmomatic's rule), then the lower density (mm1 * ov2 < mm2 * ov1), then the
 *    larger ov, then the smaller j; the order is total;
 *  - cut = c of the best, or lq where nothing is accepted; length = cut if cut >= min_length, else 0: a dropped read is an
 *    empty record, as an unmerged pair is.  The trimmed read is a[0:length] with q[0:length];
 *  - out_trims, where given, receives sassy_hip_reads_n(reads) records of 16 bytes;
 *  - *out_trimmed: an ordinary sassy_hip_Reads on the searcher's device, ONE RECORD PER READ, with qualities kept iff the input
 *    kept them.  id_start = id_len = 0 (the ids are the input's); under kept qualities qual_start = seq_start and
 *    qual_len = seq_len index the handle's own quality buffer, otherwise both are 0.  Zero reads, or nothing left of any:
 *    text_bytes == 64.  The caller frees it with sassy_hip_reads_free;
 *  - limits: at most SASSY_HIP_TRIM_MAX_ADAPTERS adapters of 1 .. 64 bytes, none shorter than min_overlap; reads of at most
 *    SASSY_HIP_OVERLAP_MAX_LEN bytes; k is not capped (k beyond 64 accepts what k = 64 does).  n_adapters == 0 is allowed:
 *    quality and length trimming only.  The searcher's rc plays no part;
 *  - refused before any device work, in this order, SASSY_HIP_EINVAL unless noted: s == NULL; any flag; min_overlap == 0;
 *    max_permille > 1000; quality_cutoff > 93; too many adapters, a null, empty or over-long adapter, an adapter shorter than
 *    min_overlap; an Ascii searcher; overhang, only_best_match, max_n_frac set (SASSY_HIP_EUNSUPPORTED); reads == NULL; a
 *    handle made on another device than the searcher's; a read longer than SASSY_HIP_OVERLAP_MAX_LEN; quality_cutoff > 0 on a
 *    handle parsed without SASSY_HIP_KEEP_QUALITY; out_trimmed == NULL; searches in flight on the searcher.  A Dna searcher
 *    takes A, C, G, T only, in the adapters and in the batch (looked at on the device, as sassy_hip_read_overlaps looks);
 *    anything else is SASSY_HIP_EINVAL and the message points to an iupac searcher.  *out_trimmed is NULL after every refusal;
 *  - the input handle is only read.  Device work on the searcher's stream: the find kernel (one wavefront per read), the layout
 *    scan of the parse over the records' lengths, one host wait for the layout's size, one write kernel indexed by 64-byte
 *    block of the output.  Stats: candidates = the reads with an adapter found, scan_launches = 5, or 6 under a Dna searcher
 *    whose batch has a block to look at (the look is a kernel as well, and is counted), word_rows = the words per plane of the
 *    find kernel's instance.  Zero reads launch no kernel: scan_launches = 0. */
#define SASSY_HIP_TRIM_MAX_ADAPTERS 64u
typedef struct sassy_hip_ReadTrim {
  uint32_t length;      /* of the trimmed read; 0: dropped by min_length (or nothing left) */
  uint32_t quality_len; /* lq */
  uint32_t adapter_pos; /* cut: c of the best position, or lq */
  int16_t adapter;      /* j of the best position; -1: no adapter found */
  uint8_t overlap;      /* its ov */
  uint8_t mismatches;   /* its mm; both 0 where no adapter was found */
} sassy_hip_ReadTrim;
int sassy_hip_trim_reads(sassy_SearcherType *s, const sassy_hip_Reads *reads, const uint8_t *const *adapters,
                         const size_t *adapter_lens, size_t n_adapters, uint32_t min_overlap, size_t k, uint32_t max_permille,
                         uint32_t quality_cutoff, uint32_t min_length, uint32_t flags,
                         sassy_hip_ReadTrim *out_trims /* may be NULL; sassy_hip_reads_n(reads) */,
                         sassy_hip_Reads **out_trimmed);

/* A window of every read as a NEW resident read batch: read r of *out is bytes [begins[r], begins[r] + lens[r]) of read r of
 * `reads` (and of its quality where kept) -- fixed clipping, a leading UMI or barcode split off.  begins and lens are host
 * arrays of sassy_hip_reads_n(reads) entries.  The layout scan and the write kernel are the trim's; the handle is as the
 * trim's (ONE RECORD PER READ, id_start = id_len = 0).  SASSY_HIP_EINVAL: a null pointer, a window that reaches outside its
 * read.  Runs on `hip_stream` on the handle's device and returns when the new handle is whole; the input is only read. */
int sassy_hip_reads_slice(const sassy_hip_Reads *reads, const uint64_t *begins, const uint64_t *lens, void *hip_stream,
                          sassy_hip_Reads **out);

/* A gather of reads as a NEW resident read batch: record j of *out is bytes [begins[j], begins[j] + lens[j]) of read src[j] of
 * `reads` (and of its quality where kept).  src, begins and lens are host arrays of n_out entries; begins and lens NULL
 * together means whole reads.  src may repeat, skip and reorder, so the call takes one sample out of a demultiplexed batch,
 * puts a mate batch into the order of another, and drops the empty records a trim or a merge leaves.  n_out may be 0.  The
 * layout scan and the write kernel are the trim's; the handle is as the trim's (id_start = id_len = 0, qualities iff the
 * source keeps them, text_bytes == 64 when nothing is left).  SASSY_HIP_EINVAL: a null pointer, only one of begins and lens,
 * src[j] >= sassy_hip_reads_n(reads), a window that reaches outside its read; the message names j.  There is no searcher: it
 * runs on `hip_stream` on the handle's device and returns when the new handle is whole; the input is only read. */
int sassy_hip_reads_select(const sassy_hip_Reads *reads, const uint64_t *src, const uint64_t *begins, const uint64_t *lens,
                           uint64_t n_out, void *hip_stream, sassy_hip_Reads **out);

/* Demultiplexing (sassy_amd/csrc/demux_reads.hip, arithmetic in demux_step.h): every read of a resident batch
 * is given to the sample whose barcode stands at a fixed place at one of its ends, and the batch comes back as a NEW resident
 * read batch SORTED BY SAMPLE with the barcode clipped off.  The definition is tests/helpers/demux_reads_ref.py.  Read a of la
 * bytes; barcodes p_0 .. p_{B-1}, all of barcode_len = m bytes.  Integers only.
 *  - WINDOW: from the 5' end w = at, under SASSY_HIP_DEMUX_END3 w = la - at - m; the read has a window iff at + m <= la;
 *  - cost_j = #{ i < m : !match(p_j[i], a[w + i]) },  match: the searcher's profile relation, the barcode on the pattern side
 *    (under Iupac an N in a barcode is a wildcard);
 *  - best = the smallest j of the minimum cost, cost = that minimum, n_best = the barcodes at that cost, second = the minimum
 *    over j != best, m + 1 when B == 1;
 *  - ASSIGNED iff the read has a window, cost <= k and second - cost >= min_delta.  min_delta == 0: a tie goes to the smaller
 *    index; min_delta >= 1: a tie is unassigned.  The label is best, or B: the unassigned bin comes last;
 *  - order = the stable argsort of the labels; out_bounds[s], s = 0 .. B + 1, is the first place of label s, so sample s is
 *    the records [out_bounds[s], out_bounds[s + 1]) of *out_sorted and the unassigned are [out_bounds[B], out_bounds[B + 1]);
 *  - record j of *out_sorted is read order[j]: an assigned read without its barcode -- bytes [at + m, la) from the 5' end (what
 *    lies in front of the barcode goes with it), [0, la - at - m) from the 3' end --, any other read whole, and every read
 *    whole under SASSY_HIP_DEMUX_KEEP_BARCODE; the quality alongside where the handle keeps one;
 *  - out_assign, where given, receives sassy_hip_reads_n(reads) records of 16 bytes in the INPUT's order; out_order, where
 *    given, as many indices; out_bounds is required and has n_barcodes + 2 entries;
 *  - *out_sorted: an ordinary sassy_hip_Reads as the trim's (id_start = id_len = 0, qual_start = seq_start under kept
 *    qualities; text_bytes == 64 when nothing is left).  Take a sample out with sassy_hip_reads_select, put a mate batch in
 *    the same order with it.  The caller frees it with sassy_hip_reads_free;
 *  - limits: 1 .. SASSY_HIP_DEMUX_MAX_BARCODES barcodes of one length 1 .. 64; at + barcode_len <= 512; min_delta <= 65; reads
 *    of at most SASSY_HIP_OVERLAP_MAX_LEN bytes; k is not capped (k beyond 64 accepts what k = 64 does).  The searcher's rc
 *    plays no part;
 *  - refused before any device work, in this order, SASSY_HIP_EINVAL unless noted: s == NULL; a flag other than the two above;
 *    min_delta > 65; n_barcodes == 0 or > 4096; barcode_len == 0 or > 64; a null barcode; at + barcode_len > 512; an Ascii
 *    searcher; overhang, only_best_match, max_n_frac set (SASSY_HIP_EUNSUPPORTED); reads == NULL; a handle made on another
 *    device than the searcher's; a read longer than SASSY_HIP_OVERLAP_MAX_LEN; out_bounds or out_sorted NULL; searches in
 *    flight on the searcher.  A Dna searcher takes A, C, G, T only, in the barcodes (looked at on the host) and in the batch
 *    (looked at on the device, as the trim looks); anything else is SASSY_HIP_EINVAL and the message points to an iupac
 *    searcher.  *out_sorted is NULL after every refusal;
 *  - the input handle is only read.  Device work on the searcher's stream: the assign kernel (a lane per read), rocPRIM's
 *    radix sort of (label, index), the bounds kernel, the place kernel, the layout scan of the parse over the new lengths, one
 *    host wait for the layout's size, the trim's write kernel with a source table.  Stats: candidates = the assigned reads,
 *    scan_launches = 8, or 9 under a Dna searcher whose batch has a block to look at: the look, the assign kernel, the sort
 *    (the library's launches count as one), bounds, place, the three kernels of the layout scan, the write kernel.  Zero
 *    reads launch no kernel: scan_launches = 0 and out_bounds is all zero. */
#define SASSY_HIP_DEMUX_MAX_BARCODES 4096u
#define SASSY_HIP_DEMUX_END3 1u         /* the barcode is counted from the 3' end */
#define SASSY_HIP_DEMUX_KEEP_BARCODE 2u /* do not clip */
typedef struct sassy_hip_ReadDemux {
  int32_t sample;  /* best where assigned; -1: unassigned */
  uint32_t best;   /* UINT32_MAX: the read has no window */
  uint8_t cost;    /* 255: no window */
  uint8_t second;  /* 255: no window */
  uint16_t n_best; /* 0: no window */
  uint32_t index;  /* where this read lies in *out_sorted: the inverse of the order */
} sassy_hip_ReadDemux;
int sassy_hip_demux_reads(sassy_SearcherType *s, const sassy_hip_Reads *reads, const uint8_t *const *barcodes, size_t barcode_len,
                          size_t n_barcodes, uint32_t at, size_t k, uint32_t min_delta, uint32_t flags,
                          sassy_hip_ReadDemux *out_assign /* may be NULL; n */, uint64_t *out_order /* may be NULL; n */,
                          uint64_t *out_bounds /* required; n_barcodes + 2 */, sassy_hip_Reads **out_sorted);

/* UMI grouping and deduplication of a resident read batch (sassy_amd/csrc/dedup_reads.hip, arithmetic in dedup_step.h;
 * DESIGN.md 5.8h): sassy_hip_umi_groups over a window of every read, with no byte of the batch leaving the device, and of
 * every group ONE read kept, as a NEW resident read batch.  The definition is tests/helpers/dedup_reads_ref.py.  Integers only.
 *  - KEY: the key of read r, of la bytes, is its window of m bytes at w; from the 5' end w = at, under SASSY_HIP_DEDUP_END3
 *    w = la - at - m (the demux's window).  It may be a UMI alone or a UMI and the first bases of the insert: the call does not
 *    care.  A read with la < at + m has no window and takes no part: its label and rep are UINT32_MAX, its size and count 0,
 *    and it is never kept;
 *  - GROUPS: let r_0 < r_1 < ... be the reads that have a window.  The four columns, *n_unique and *n_groups are exactly what
 *    sassy_hip_umi_groups returns for the host list of their windows under the same searcher, k and method, every index j of
 *    that result mapped to r_j (ascending order is kept, so "smallest index" stays smallest).  An rc searcher: neighbours on
 *    either strand, as there.  k >= m is cut to m;
 *  - KEPT READ (sassy_hip_dedup_reads): of every group the member with the highest score, on a tie the smallest index; the
 *    score is the sum of the read's raw quality bytes where the handle keeps qualities, otherwise the read's length -- as one
 *    64-bit key, score << 32 | (0xFFFFFFFF - r), maximised.  out_kept (may be NULL; n entries, the first *n_groups written)
 *    lists the kept reads in ascending read index; record j of *out_dedup is read out_kept[j] whole: the handle
 *    sassy_hip_reads_select makes for src = out_kept (id_start = id_len = 0, qualities iff the source keeps them,
 *    text_bytes == 64 when nothing is kept).  The caller frees it with sassy_hip_reads_free;
 *  - the columns have sassy_hip_reads_n(reads) entries.  sassy_hip_umi_groups_reads requires out_label; in
 *    sassy_hip_dedup_reads all four may be NULL.  n_unique and n_groups may be NULL;
 *  - limits: 1 <= m <= 128; at + m <= 512; reads of at most SASSY_HIP_OVERLAP_MAX_LEN bytes; at most 2^31 - 1 reads
 *    (SASSY_HIP_EUNSUPPORTED beyond);
 *  - refused before any device work, in this order, SASSY_HIP_EINVAL unless noted: s == NULL; a flag other than
 *    SASSY_HIP_DEDUP_END3; an unknown method; m == 0 or m > 128; at + m > 512; an Ascii searcher (use a dna or an iupac one);
 *    overhang, only_best_match, max_n_frac set (SASSY_HIP_EUNSUPPORTED); reads == NULL; a handle made on another device than
 *    the searcher's; a read longer than SASSY_HIP_OVERLAP_MAX_LEN; out_label NULL (the groups call), out_dedup NULL (the dedup
 *    call); searches in flight on the searcher.  A Dna searcher takes batches of A, C, G, T only, looked at on the device as
 *    the trim looks; anything else is SASSY_HIP_EINVAL and the message points to an iupac searcher.  *out_dedup is NULL after
 *    every refusal;
 *  - zero reads, or no read with a window (the handle's longest read is shorter than at + m): success, no kernel launched,
 *    the counts zero, the columns the sentinels, an empty handle;
 *  - the input handle is only read.  Device work on the searcher's stream: the flag kernel, a scan, one host wait for the
 *    count, the encode kernel (a lane per read: the window into the pair family's bit planes), sassy_hip_umi_groups' device
 *    part over those planes, the scatter kernel; the dedup call then: the score kernel (one 64-bit atomic max per read), the
 *    keep kernel, a scan, one host wait, a compaction, the layout scan of the parse, the trim's write kernel with a source
 *    table;
 *  - sassy_hip_get_stats afterwards: everything sassy_hip_umi_groups leaves (filtered = 12, candidates, hit_blocks = n_unique,
 *    blocks, chunks, grid, the three timing spans at level 2), text_bytes = windows x m, and scan_launches = what that call's
 *    walk leaves there (0 UNIQUE, 1 CLUSTER, DIRECTIONAL 1 or 2: 2 where the distinct keys have a pair record) plus this
 *    unit's own launches: 6 for the groups call (flag, the scan's three, encode, scatter), 16 for the dedup call (those and
 *    score, keep, the scan's three, compaction, the layout scan's three, write), one more under a Dna searcher whose batch
 *    has a block to look at.  Zero reads or no window: scan_launches = 0. */
#define SASSY_HIP_DEDUP_END3 1u   /* the window is counted from the 3' end */
int sassy_hip_umi_groups_reads(sassy_SearcherType *s, const sassy_hip_Reads *reads, uint32_t at, size_t m, size_t k,
                               uint32_t method, uint32_t flags,
                               uint32_t *out_label, uint32_t *out_size, uint32_t *out_rep, uint32_t *out_count, /* n each */
                               size_t *n_unique, size_t *n_groups);
int sassy_hip_dedup_reads(sassy_SearcherType *s, const sassy_hip_Reads *reads, uint32_t at, size_t m, size_t k,
                          uint32_t method, uint32_t flags,
                          uint32_t *out_label, uint32_t *out_size, uint32_t *out_rep, uint32_t *out_count, /* may all be NULL here */
                          uint64_t *out_kept /* may be NULL; n entries, the first *n_groups written */,
                          size_t *n_unique, size_t *n_groups, sassy_hip_Reads **out_dedup);

/* One row of the reference CLI's match table (bin/grep.rs:465-470 header, :710-757 rows):
 *   pat_id  text_id  cost  strand  start  end  match_region  cigar
 * match_region = text[start..end), reverse-complemented for Rc matches unless `sam`; the cigar is
 * reversed for Rc matches if `sam`.  `m` is a match record, `cigar` its NUL-terminated cigar text
 * (sassy_hip_result_cigars(r) + m->cigar_off), `text` the host copy of the text it refers to.
 * Writes at most cap bytes (NUL-terminated, '\n'-terminated row) and returns the length the full
 * row needs (excluding the NUL), or a negative error code.  sassy_hip_tsv_header() is the header line. */
const char *sassy_hip_tsv_header(void);
long sassy_hip_format_tsv(const sassy_SearcherType *s, const sassy_hip_Match *m, const char *cigar,
                          const char *pat_id, const char *text_id, const uint8_t *text,
                          size_t text_len, int sam, char *buf, size_t cap);

/* One shard of a larger text that lives on this device (multi-GPU).
 * d_text points at the first byte of the halo; the shard owns global end positions whose
 * 64-byte block lies in [global_offset, global_offset + shard_len); halo_len bytes precede it
 * (halo_len = 0 for the first shard, otherwise >= sassy_hip_required_halo(m, k); halo_len,
 * global_offset and -- except for the last shard -- shard_len are multiples of 64).
 * total_len is the length of the whole text (the end-of-text rule is applied by the shard that
 * contains it).  Matches carry global coordinates.  Forward strand only. */
int sassy_hip_search_shard(sassy_SearcherType *s, const uint8_t *pattern, size_t pattern_len,
                           const uint8_t *d_text, uint64_t halo_len, uint64_t shard_len,
                           uint64_t global_offset, uint64_t total_len, size_t k, uint32_t flags,
                           sassy_hip_Result **out);
uint64_t sassy_hip_required_halo(size_t pattern_len, size_t k);

/* Searches in flight.  A stream of searches over a resident text (many patterns against one genome; the
 * reference's model is one Searcher per thread fed from a queue, bin/grep.rs:476-503) is pipelined on the
 * device: sassy_hip_search_shard_begin queues the whole kernel chain of one search (same arguments and rules
 * as sassy_hip_search_shard) and returns a ticket at once; sassy_hip_search_finish waits for that search and
 * hands out its result (out = NULL: wait and discard).  Up to 2 searches (sassy_hip_set_pipe_depth, at most 4) may
 * be in flight per searcher -- begin fails with SASSY_HIP_EINVAL beyond that --; they finish in any order the
 * caller likes, each result is exactly what sassy_hip_search_shard returns.  The short, latency-bound tail of
 * search i (chunk list, chunk DP, traceback) then runs underneath the bandwidth-bound prefilter of search
 * i+1.  The pattern is copied; the text must stay valid and unchanged until the ticket is finished.  Every
 * ticket must be finished before the searcher is freed (tickets still open then are dropped).
 * Searches in flight may share their text pass: a Dna forward search on the fused bit-plane path can be served together
 * with a second such search over the same buffer (same d_text, halo_len, shard_len, global_offset, total_len, flags
 * and piece length, at most 8 pieces together) by one launch that filters the text for both
 * (sassy_hip_Stats.pass_patterns = 2).  The pass of such a search is cut in two halves of its grid: a begin launches the
 * previous search's second half together with this search's first half, so a search is complete one begin after its
 * own and a launch is always queued behind the running one.  A search that finds neither a partner nor a pass
 * streaming is launched whole; a search that cannot share is begun behind what the open ones still need; finish
 * launches what its own ticket still needs -- no ticket waits on a launch that only a later call would make.
 * Results are unchanged; SASSY_HIP_SHARED_PASS=0
 * (sassy_hip_set_option "shared_pass") turns it off.
 * Kept code planes.  Because the text may not change while a ticket is open, what a pass derives from the text alone --
 * the two code bit planes of every 64-byte block, 16 bytes -- is kept across such searches: the first launch over a half
 * of the grid stores them, the launches behind it read them instead of the text (sassy_hip_Stats.plane_launches).  The
 * planes live exactly as long as the searcher has had at least one ticket open without a break: when the last open ticket
 * is finished they are forgotten, and the caller may rewrite the buffer as before; the flag SASSY_HIP_TEXT_UNCHANGED
 * does not extend that.  Only tickets of one buffer and geometry use them at a time; a ticket over another buffer
 * or shard in between reads its text as ever.  The store costs a quarter of the text (0.76 GB of device memory for 3 GB),
 * is allocated per searcher at the first launch that can use it, reused while it is large enough and freed with the
 * searcher; if it cannot be allocated, or is larger than the switch plane_cache_max_mb allows, nothing is kept.
 * Planes are written only where a reader can follow: a search begun and finished with nothing else in flight takes its
 * own launch, and no store is made for it.
 * SASSY_HIP_PLANE_CACHE=0 (sassy_hip_set_option "plane_cache") turns it off.  The calls of
 * one searcher must still come from one thread at a time.  sassy_hip_get_stats describes the search finished last.
 * While a ticket is open the searcher's synchronous entry points (sassy_hip_search, _search_shard, _search_many,
 * _search_encoded, _search_with_fn, the drop-in search) and sassy_hip_set_stream fail with SASSY_HIP_EINVAL: they
 * use the same streams and result buffers. */
/* The results of consecutive shards of one text (results[0] the leftmost), merged into one: matches in text order
 * with their cigars; a shard's conditional report (sassy_hip_result_conditional_index) is kept iff the plateau
 * state arriving from the shards on its left is TRUE (exit states, PASS = "ask further left").  incoming_state is the
 * state in front of results[0]: 1 (TRUE) when results[0] begins the text, 2 (PASS) when that is unknown -- then a
 * conditional report of the first shards stays conditional in the merged result, whose exit state and conditional
 * index make it a shard result again (merges nest).  This is what sassy_amd/multigpu.py does with gathered rows; a C
 * or Rust host that searched its shards with sassy_hip_search_shard on several devices calls it directly. */
int sassy_hip_merge_shards(const sassy_hip_Result *const *results, size_t n, int incoming_state, sassy_hip_Result **out);

/* One text over several devices inside one process (the reference's thread fan-out, bin/grep.rs:476-503, with a
 * GPU per thread): the text is cut into as many shards of whole 64-byte blocks as there are entries in `devices`
 * (NULL / 0: every visible device; a device may be named more than once -- several shards on one GPU), every shard
 * resident on its device with sassy_hip_required_halo(max_pattern_len, max_k) bytes of the text in front of it.  Each
 * device has a host thread of its own: sassy_hip_multi_set_text uploads all shards at once (one PCIe link per
 * device), sassy_hip_multi_search runs sassy_hip_search_shard on all devices at once and merges
 * (sassy_hip_merge_shards).  Forward strand, like the shard calls; flags: SASSY_HIP_ALL_MINIMA,
 * SASSY_HIP_WITHOUT_TRACE.  alpha = NAN (overhang needs the whole text in one buffer).  One call at a time per
 * multi-searcher. */
typedef struct sassy_hip_Multi sassy_hip_Multi;
sassy_hip_Multi *sassy_hip_multi_new(const char *alphabet, float alpha, const int *devices, size_t n_devices);
size_t sassy_hip_multi_shards(const sassy_hip_Multi *m);
int sassy_hip_multi_device(const sassy_hip_Multi *m, size_t shard);
sassy_SearcherType *sassy_hip_multi_searcher(sassy_hip_Multi *m, size_t shard); /* (for the setters; owned by m) */
int sassy_hip_multi_set_text(sassy_hip_Multi *m, const uint8_t *text, size_t len, size_t max_pattern_len, size_t max_k);
/* the synthetic text of sassy_hip_generate_dna / sassy_hip_plant, every device generating its own shard in place */
int sassy_hip_multi_generate_dna(sassy_hip_Multi *m, uint64_t len, uint64_t seed, size_t max_pattern_len, size_t max_k);
int sassy_hip_multi_plant(sassy_hip_Multi *m, uint64_t seed, const uint8_t *pattern, size_t pattern_len, size_t k,
                          uint64_t stride, uint64_t *planted);
int sassy_hip_multi_search(sassy_hip_Multi *m, const uint8_t *pattern, size_t pattern_len, size_t k, uint32_t flags,
                           sassy_hip_Result **out);
/* Both strands (reference: Searcher::new_rc; the CLI's default, bin/grep.rs:476-503 fans such searches out over its
 * threads): sassy_hip_multi_search then appends the Rc strand's matches to the forward ones, as sassy_hip_search does.
 * The Rc strand is complement(pattern) against the REVERSED text (src/search.rs:813-878): every device keeps a few
 * bytes of text on BOTH sides of its shard and searches its share of the reversed text as a shard of its own
 * (reversed with the reverse kernel, never uploaded twice); the shard results are chained in reversed order. */
int sassy_hip_multi_set_rc(sassy_hip_Multi *m, int rc);
/* search_encoded_patterns over several devices shards the PATTERNS (bin/crispr.rs:188-196): every device
 * scans the whole text for its share -- no halo, no seam, the same gather.  That needs the whole text on every device:
 * call sassy_hip_multi_set_replicated(m, 1) BEFORE the text is set / generated (0 = text shards again).  The result's
 * pattern_idx refers to the caller's list; order: device by device (the reference's order is an implementation
 * artefact too -- compare sorted).  Both strands with sassy_hip_multi_set_rc. */
int sassy_hip_multi_set_replicated(sassy_hip_Multi *m, int on);
int sassy_hip_multi_search_encoded(sassy_hip_Multi *m, const uint8_t *patterns, size_t n_patterns, size_t pattern_len,
                                   size_t k, uint32_t flags, sassy_hip_Result **out);
/* search_many over several devices shards the TEXTS (host pointers; whole texts, contiguous runs of about equal total
 * length per device; src/search.rs:531-603 does the same over threads): every device searches all patterns in its
 * texts, text_idx refers to the caller's list.  Needs no resident text.  (There is no multi-device sassy_hip_min_costs /
 * _best_pattern: shard the texts over one searcher per device -- each fills its own columns.) */
int sassy_hip_multi_search_many(sassy_hip_Multi *m, const uint8_t *const *patterns, const size_t *pattern_lens,
                                size_t n_patterns, const uint8_t *const *texts, const size_t *text_lens, size_t n_texts,
                                size_t k, uint32_t flags, sassy_hip_Result **out);
/* Searches in flight over several devices (the reference's worker threads never idle between two tasks,
 * bin/grep.rs:516-537, src/search.rs:531-603): begin() queues one shard search per device and strand
 * (sassy_hip_search_shard_begin on every device's host thread) and returns; finish() waits for that search on every
 * device and merges the shard results -- the tail of search i (chunk DP, tracebacks, the host's merge) runs under the
 * text stream of search i + 1 on every device.  Up to `depth` searches per multi-searcher (1 .. 4, default 3); tickets
 * may be finished in any order.  While a ticket is open every entry point that rewrites, re-lays-out or reallocates the
 * resident shards or uses the devices' searchers is refused with SASSY_HIP_EINVAL: sassy_hip_multi_set_text,
 * _generate_dna, _plant, _set_rc, _set_replicated, _search, _search_encoded and _search_many (the searches in flight
 * read those buffers).  Same result as sassy_hip_multi_search, both strands included (sassy_hip_multi_set_rc). */
typedef struct sassy_hip_MultiTicket sassy_hip_MultiTicket;
int sassy_hip_multi_set_pipe_depth(sassy_hip_Multi *m, int depth);
int sassy_hip_multi_search_begin(sassy_hip_Multi *m, const uint8_t *pattern, size_t pattern_len, size_t k,
                                 uint32_t flags, sassy_hip_MultiTicket **out);
int sassy_hip_multi_search_finish(sassy_hip_Multi *m, sassy_hip_MultiTicket *t, sassy_hip_Result **out);
/* The layout arithmetic of a multi-searcher without any device: part i's {offset, len, halo in front, bytes kept
 * behind, first / one-past-last forward byte of its share of the REVERSED text, that share's halo} in
 * out[7 i .. 7 i + 6] (out may be NULL).  Returns the number of parts that hold a share of the text (a text of less
 * than 64 n (n + 2) bytes is one device's), or -1 if a part's resident bytes would not cover its share of the
 * reversed text (never, by construction: what the tests pin). */
long sassy_hip_multi_layout(uint64_t len, size_t n_parts, size_t max_pattern_len, size_t max_k, uint64_t *out);
/* Where the seeded search of sassy_hip_search_encoded (many patterns, a long text) puts its seeds: k + 1 disjoint
 * pieces of the pattern's rows -- out_end[i] = one past the last row, out_len[i] = rows (<= 10) -- of at most two
 * lengths; with ambiguity letters in the patterns (alphabet "iupac") placed where the expected number of table
 * hits is smallest.  Host arithmetic, no device (tests).  Returns k + 1, or -1 for arguments out of range
 * (pattern_len 1 .. 64, k <= 7, k + 1 <= pattern_len). */
long sassy_hip_seed_layout(const char *alphabet, const uint8_t *const *patterns, size_t n_patterns, size_t pattern_len,
                           size_t k, uint32_t *out_end, uint32_t *out_len);
/* The 64 table rows of the sub-piece test that runs in front of the seeded search's verification, for seeds
 * (seed_end[i], seed_len[i]), i <= k, of a pattern of pattern_len <= 32 rows: out_rows[8 p + u] = 2a | (32 - 2 len) << 8 |
 * 2 (off & 15) << 16 | (off >> 4) << 24 for sub-piece u (rows [a, a + len)) of piece p, off = its leftmost shift in
 * characters from the start of the one text window the test reads (*out_win_left characters in front of the seed's
 * end); low byte 0xFF in out_rows[8 p]: no test for piece p.  Returns the largest off (<= 47), -1 for arguments out
 * of range.  Host arithmetic, no device (tests). */
long sassy_hip_seed_test_rows(size_t pattern_len, size_t k, const uint32_t *seed_end, const uint32_t *seed_len,
                              uint32_t *out_rows, uint32_t *out_win_left);
void sassy_hip_multi_free(sassy_hip_Multi *m);

typedef struct sassy_hip_Ticket sassy_hip_Ticket;
int sassy_hip_search_shard_begin(sassy_SearcherType *s, const uint8_t *pattern, size_t pattern_len,
                                 const uint8_t *d_text, uint64_t halo_len, uint64_t shard_len,
                                 uint64_t global_offset, uint64_t total_len, size_t k, uint32_t flags,
                                 sassy_hip_Ticket **out);
int sassy_hip_search_finish(sassy_SearcherType *s, sassy_hip_Ticket *ticket, sassy_hip_Result **out);
/* How many searches sassy_hip_search_shard_begin keeps in flight (1 .. 4, default 2 or SASSY_HIP_PIPE_DEPTH);
 * only while none is in flight. */
int sassy_hip_set_pipe_depth(sassy_SearcherType *s, int depth);

size_t sassy_hip_result_len(const sassy_hip_Result *r);
const sassy_hip_Match *sassy_hip_result_matches(const sassy_hip_Result *r);
const sassy_hip_LineSpan *sassy_hip_result_line_spans(const sassy_hip_Result *r); /* NULL unless SASSY_HIP_LINE_SPANS was set */
const char *sassy_hip_result_cigars(const sassy_hip_Result *r); /* string pool */
size_t sassy_hip_result_cigars_len(const sassy_hip_Result *r);   /* bytes in the pool */
/* Wire format of the multi-GPU match gather (sassy_amd/multigpu.py): one row of 7 + cigar_bytes/8
 * int64 per match -- pattern_idx, text_start, text_end, pattern_start, pattern_end, cost, strand, then
 * cigar_bytes bytes of NUL-padded cigar text.  Pure host helper (no device needed); `cigar_bytes` is a
 * multiple of 8.  SASSY_HIP_EINVAL if a cigar string does not fit. */
int sassy_hip_pack_rows(const sassy_hip_Match *matches, size_t n, const char *cigars, size_t cigars_len,
                        int64_t *rows, size_t cigar_bytes);
/* Shard bookkeeping for the cross-shard plateau rule (see DESIGN.md "seams"):
 * entry_state: 0 = the shard's first report did not depend on the previous shard,
 *              1 = it did (the record with SASSY flag is still in the result, marked below);
 * exit_state:  0 = decreasing FALSE, 1 = decreasing TRUE, 2 = PASS (undetermined, inherit). */
int sassy_hip_result_exit_state(const sassy_hip_Result *r);
int64_t sassy_hip_result_conditional_index(const sassy_hip_Result *r); /* -1 if none */
void sassy_hip_result_free(sassy_hip_Result *r);

/* Searcher::encode_patterns / search_encoded_patterns (src/search.rs:404-423):
 * npat patterns of equal length plen (<= 64) stored back to back.
 * The many-pattern calls (this one and sassy_hip_search_many): the reports are the definition's (one left-to-right
 * pass per pattern and text) -- as in the reference, whose lanes hold whole texts / patterns there (no lane seams:
 * sassy_hip_set_reference_lanes has nothing to reproduce).  An overhang searcher (alpha) takes one pass as well where
 * the shape allows it (>= 4 Iupac patterns of one length <= 64 with seeds, plain-base text: the seeded search lists the
 * inside of the text, the per-text tiled scan its two edges; the reference's v2 scans overhang in its tiled loop,
 * src/pattern_tiling/search.rs:222-323); other overhang shapes run one kernel chain per pattern. */
sassy_hip_Encoded *sassy_hip_encode_patterns(sassy_SearcherType *s, const uint8_t *patterns,
                                             size_t npat, size_t plen);
void sassy_hip_encoded_free(sassy_hip_Encoded *e);
int sassy_hip_search_encoded(sassy_SearcherType *s, const sassy_hip_Encoded *e,
                             const uint8_t *text, size_t text_len, size_t k, uint32_t flags,
                             sassy_hip_Result **out);

/* Synthetic inputs generated in place on the device; same function as
 * oracle/sassy_oracle.c:orc_generate_dna / orc_plant_window, checked byte for byte in tests. */
int sassy_hip_generate_dna(uint8_t *d_text, uint64_t n, uint64_t seed, uint64_t first,
                           void *hip_stream);
/* A repeat-rich synthetic text (measurement and test input, like sassy_hip_generate_dna): 4 KiB regions of
 * i.i.d. ACGT (the majority), microsatellites (6 %), copies of 4 interspersed-repeat families with 8 %
 * divergence (10 %), soft-masked stretches (1 %) and, with with_n != 0, runs of 'N' (2 %); every byte is a pure
 * function of (seed, first + index).  See sassy_amd/csrc/aux_kernels.hip: genome_like_byte. */
int sassy_hip_generate_genome_like(uint8_t *d_text, uint64_t n, uint64_t seed, uint64_t first, int with_n,
                                   void *hip_stream);
int sassy_hip_plant(uint8_t *d_text, uint64_t n, uint64_t first, uint64_t total_n, uint64_t seed,
                    const uint8_t *pattern, size_t pattern_len, size_t k, uint64_t stride,
                    void *hip_stream, uint64_t *planted);
/* ... with the plants `phase` bytes further on (q * stride + stride / 2 + phase): several patterns in one text. */
int sassy_hip_plant_phase(uint8_t *d_text, uint64_t n, uint64_t first, uint64_t total_n, uint64_t seed,
                          const uint8_t *pattern, size_t pattern_len, size_t k, uint64_t stride, uint64_t phase,
                          void *hip_stream, uint64_t *planted);

/* Plain device memory helpers so that non-torch callers (C, tests) can use the device paths. */
void *sassy_hip_malloc(size_t bytes);
void sassy_hip_free(void *d_ptr);
int sassy_hip_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes);
int sassy_hip_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SASSY_HIP_H */
