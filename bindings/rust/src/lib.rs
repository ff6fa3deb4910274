//! Rust host side of the MI355X search path: the reference's `Searcher<P>` surface
//! (`/root/reference/src/search.rs:227-784`: `new_fwd`, `new_rc`, `search`, `search_all`,
//! `encode_patterns`, `search_encoded_patterns`) forwarded through the C-ABI of `include/sassy_hip.h`.
//!
//! SOURCE ONLY: the image this repository is built in has no `rustc` / `cargo`; nothing in the test
//! suite compiles this file.  Every `extern "C"` item below is a declaration of `include/sassy_hip.h`;
//! the C client `tests/c/dropin_client.c` and the Python `ctypes` layer exercise the same symbols.
use std::ffi::{c_char, c_int, c_long, CStr, CString};
use std::marker::PhantomData;

#[repr(C)]
struct RawMatch {
    // include/sassy_hip.h: sassy_hip_Match (64 bytes)
    pattern_idx: u64,
    text_idx: u64,
    text_start: u64,
    text_end: u64,
    pattern_start: u64,
    pattern_end: u64,
    cost: i32,
    strand: u8,
    _pad: [u8; 3],
    cigar_off: u32,
    cigar_len: u32,
}
/// One product of a primer pair (include/sassy_hip.h: sassy_hip_Amplicon, 24 bytes): `strand` 0 = fwd on the forward strand
/// at `start`, 1 = rev; `fwd_cost` / `rev_cost` are the mismatches of fwd and of rev, whichever side they sit on.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Amplicon {
    pub start: u64,
    pub end: u64,
    pub pair_idx: u32,
    pub strand: u8,
    pub fwd_cost: u8,
    pub rev_cost: u8,
    _pad: u8,
}
/// One pair of `hamming_pairs` (include/sassy_hip.h: sassy_hip_HammingPair, 12 bytes): sequence `a_idx` of the first list and
/// `b_idx` of the second differ in `cost` rows; `strand` 1: `b_idx` was taken as its reverse complement.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct HammingPair {
    pub a_idx: u32,
    pub b_idx: u32,
    pub cost: u8,
    pub strand: u8,
    _pad: [u8; 2],
}
/// One record of an unwrapped FASTA chunk (include/sassy_hip.h: sassy_hip_FastaRecord, 32 bytes): the id in the raw bytes,
/// the sequence in the device text.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct FastaRecord {
    pub id_start: u64,
    pub id_len: u64,
    pub seq_start: u64,
    pub seq_len: u64,
}
#[repr(C)]
pub struct RawFasta {
    _p: [u8; 0],
}
/// One read of a FASTQ chunk parsed on the device (include/sassy_hip.h: sassy_hip_ReadRecord, 48 bytes): id and quality in
/// the raw bytes, the sequence in the device text.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct ReadRecord {
    pub id_start: u64,
    pub id_len: u64,
    pub seq_start: u64,
    pub seq_len: u64,
    pub qual_start: u64,
    pub qual_len: u64,
}
#[repr(C)]
pub struct RawReads {
    _p: [u8; 0],
}
/// The best overlap of one read pair (include/sassy_hip.h: sassy_hip_ReadOverlap, 16 bytes); n_accepted == 0: no overlap, every
/// field is 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct ReadOverlap {
    pub offset: i32,
    pub overlap: u32,
    pub mismatches: u32,
    pub n_accepted: u32,
}
/// What the trim leaves of one read (include/sassy_hip.h: sassy_hip_ReadTrim, 16 bytes); adapter == -1: no adapter found.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct ReadTrim {
    pub length: u32,
    pub quality_len: u32,
    pub adapter_pos: u32,
    pub adapter: i16,
    pub overlap: u8,
    pub mismatches: u8,
}
pub const TRIM_MAX_ADAPTERS: u32 = 64;
/// Which sample one read went to (include/sassy_hip.h: sassy_hip_ReadDemux, 16 bytes); sample == -1: unassigned,
/// best == u32::MAX: the read has no window.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct ReadDemux {
    pub sample: i32,
    pub best: u32,
    pub cost: u8,
    pub second: u8,
    pub n_best: u16,
    pub index: u32,
}
pub const DEMUX_MAX_BARCODES: u32 = 4096;
pub const DEMUX_END3: u32 = 1;
pub const DEMUX_KEEP_BARCODE: u32 = 2;
pub const DEDUP_END3: u32 = 1;
#[repr(C)]
struct RawSearcher {
    _p: [u8; 0],
}
#[repr(C)]
struct RawMultiTicket {
    _p: [u8; 0],
}
#[repr(C)]
struct RawResult {
    _p: [u8; 0],
}
#[repr(C)]
struct RawEncoded {
    _p: [u8; 0],
}
#[repr(C)]
struct RawTicket {
    _p: [u8; 0],
}

pub const ALL_MINIMA: u32 = 1;
pub const WITHOUT_TRACE: u32 = 2;
pub const TEXT_ON_DEVICE: u32 = 4;
/// sassy_hip_fastq_parse only: keep the base qualities on the device (sassy_hip_reads_quality)
pub const KEEP_QUALITY: u32 = 32;
/// `min_costs` / `best_pattern`: no match of cost <= k.
pub const NO_MATCH: u8 = 255;

extern "C" {
    fn sassy_hip_searcher_new(alphabet: *const c_char, rc: bool, alpha: f32) -> *mut RawSearcher;
    fn sassy_searcher_free(s: *mut RawSearcher);
    fn sassy_hip_last_error() -> *const c_char;
    fn sassy_hip_search(s: *mut RawSearcher, pattern: *const u8, pattern_len: usize, text: *const u8,
                        text_len: usize, k: usize, flags: u32, out: *mut *mut RawResult) -> c_int;
    // character-class patterns (include/sassy_hip.h): 32 bytes per position, byte c at bit c & 7 of sets[32 j + (c >> 3)]
    fn sassy_hip_search_classes(s: *mut RawSearcher, sets: *const u8, m: usize, text: *const u8, text_len: usize,
                                k: usize, flags: u32, out: *mut *mut RawResult) -> c_int;
    fn sassy_hip_class_cover(set: *const u8, value: *mut u8, care: *mut u8, cap: usize, complemented: *mut c_int) -> c_long;
    // Hamming search (include/sassy_hip.h): every start with at most k mismatches of every pattern, one text
    fn sassy_hip_search_hamming(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                text: *const u8, text_len: usize, k: usize, flags: u32, out: *mut *mut RawResult) -> c_int;
    // ... over a batch of texts: every hit with its text_idx / per text the best (cost, pattern, strand, start), no records
    fn sassy_hip_search_hamming_many(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                     texts: *const *const u8, text_lens: *const usize, n_texts: usize, k: usize, flags: u32,
                                     out: *mut *mut RawResult) -> c_int;
    fn sassy_hip_hamming_best_pattern(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                      texts: *const *const u8, text_lens: *const usize, n_texts: usize, k: usize, flags: u32,
                                      out_cost: *mut u8, out_pattern: *mut u32, out_strand: *mut u8, out_start: *mut u64) -> c_int;
    // ... counted, not listed: out_counts[(2 p + strand) (k + 1) + c] = records with that pattern, strand and cost
    fn sassy_hip_hamming_counts(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                text: *const u8, text_len: usize, k: usize, flags: u32, out_counts: *mut u64) -> c_int;
    fn sassy_hip_hamming_counts_many(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                     texts: *const *const u8, text_lens: *const usize, n_texts: usize, k: usize, flags: u32,
                                     out_counts: *mut u64) -> c_int;
    // ... joined: the products of primer pairs (in-silico PCR), records freed with sassy_hip_amplicons_free
    fn sassy_hip_hamming_amplicons(s: *mut RawSearcher, fwd: *const *const u8, fwd_lens: *const usize, rev: *const *const u8,
                                   rev_lens: *const usize, n_pairs: usize, text: *const u8, text_len: usize, k: usize, min_len: u64,
                                   max_len: u64, flags: u32, out: *mut *mut Amplicon, n_out: *mut usize) -> c_int;
    fn sassy_hip_amplicons_free(p: *mut Amplicon);
    // ... without a text: two lists of sequences of one length all against all (b null and n_b 0: a against itself)
    fn sassy_hip_hamming_pairs(s: *mut RawSearcher, a: *const u8, n_a: usize, b: *const u8, n_b: usize, m: usize, k: usize,
                               flags: u32, out: *mut *mut HammingPair, n_out: *mut usize) -> c_int;
    fn sassy_hip_hamming_pairs_free(p: *mut HammingPair);
    fn sassy_hip_hamming_nearest(s: *mut RawSearcher, a: *const u8, n_a: usize, b: *const u8, n_b: usize, m: usize, k: usize,
                                 flags: u32, out_cost: *mut u8, out_index: *mut u32, out_strand: *mut u8, out_ties: *mut u32) -> c_int;
    // ... and under the edit distance: a length per list (sassy_hip_EditPair is sassy_hip_HammingPair, cost = E)
    fn sassy_hip_edit_pairs(s: *mut RawSearcher, a: *const u8, n_a: usize, m_a: usize, b: *const u8, n_b: usize, m_b: usize, k: usize,
                            flags: u32, out: *mut *mut HammingPair, n_out: *mut usize) -> c_int;
    fn sassy_hip_edit_pairs_free(p: *mut HammingPair);
    fn sassy_hip_edit_nearest(s: *mut RawSearcher, a: *const u8, n_a: usize, m_a: usize, b: *const u8, n_b: usize, m_b: usize, k: usize,
                              flags: u32, out_cost: *mut u8, out_index: *mut u32, out_strand: *mut u8, out_ties: *mut u32) -> c_int;
    // ... and the groups one list forms: per sequence the smallest index of its connected component within k, and its size
    fn sassy_hip_hamming_clusters(s: *mut RawSearcher, a: *const u8, n: usize, m: usize, k: usize, flags: u32, out_label: *mut u32,
                                  out_size: *mut u32, n_clusters: *mut usize) -> c_int;
    fn sassy_hip_edit_clusters(s: *mut RawSearcher, a: *const u8, n: usize, m: usize, k: usize, flags: u32, out_label: *mut u32,
                               out_size: *mut u32, n_clusters: *mut usize) -> c_int;
    // ... and UMI groups: duplicates collapsed, then method 0 unique / 1 cluster / 2 directional over the distinct sequences
    fn sassy_hip_umi_groups(s: *mut RawSearcher, a: *const u8, n: usize, m: usize, k: usize, method: u32, flags: u32, out_label: *mut u32,
                            out_size: *mut u32, out_rep: *mut u32, out_count: *mut u32, n_unique: *mut usize, n_groups: *mut usize) -> c_int;
    // FASTA unwrap on the device: raw bytes in, a device text per record and a host table out (flags: TEXT_ON_DEVICE)
    pub fn sassy_hip_fasta_unwrap(raw: *const u8, n: u64, flags: u32, hip_stream: *mut std::ffi::c_void, out: *mut *mut RawFasta) -> c_int;
    pub fn sassy_hip_fasta_n_records(f: *const RawFasta) -> u64;
    pub fn sassy_hip_fasta_records(f: *const RawFasta) -> *const FastaRecord;
    pub fn sassy_hip_fasta_text(f: *const RawFasta) -> *mut std::ffi::c_void;
    pub fn sassy_hip_fasta_text_bytes(f: *const RawFasta) -> u64;
    pub fn sassy_hip_fasta_free(f: *mut RawFasta);
    // FASTQ parse on the device: raw bytes in, a resident read batch and a host table out (flags: TEXT_ON_DEVICE) ...
    pub fn sassy_hip_fastq_parse(raw: *const u8, n: u64, flags: u32, hip_stream: *mut std::ffi::c_void, out: *mut *mut RawReads) -> c_int;
    pub fn sassy_hip_reads_n(r: *const RawReads) -> u64;
    pub fn sassy_hip_reads_records(r: *const RawReads) -> *const ReadRecord;
    pub fn sassy_hip_reads_text(r: *const RawReads) -> *mut std::ffi::c_void;
    pub fn sassy_hip_reads_text_bytes(r: *const RawReads) -> u64;
    pub fn sassy_hip_reads_longest(r: *const RawReads) -> u64;
    pub fn sassy_hip_reads_rem(r: *const RawReads) -> *const u32;
    /// the device pointer of the qualities in the text's layout; null unless the batch was parsed with KEEP_QUALITY (32)
    pub fn sassy_hip_reads_quality(r: *const RawReads) -> *const u8;
    pub fn sassy_hip_reads_free(r: *mut RawReads);
    // ... and the Hamming batch calls over it: the handle where the _many sibling takes texts, text_lens, n_texts
    fn sassy_hip_search_hamming_reads(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                      reads: *const RawReads, k: usize, flags: u32, out: *mut *mut RawResult) -> c_int;
    fn sassy_hip_hamming_best_pattern_reads(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                            reads: *const RawReads, k: usize, flags: u32, out_cost: *mut u8, out_pattern: *mut u32,
                                            out_strand: *mut u8, out_start: *mut u64) -> c_int;
    fn sassy_hip_hamming_counts_reads(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                      reads: *const RawReads, k: usize, flags: u32, out_counts: *mut u64) -> c_int;
    // ... and the edit-distance batch calls: the resident reads are laid out for the scan by a kernel, no upload
    pub fn sassy_hip_search_many_reads(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                       reads: *const RawReads, k: usize, flags: u32, out: *mut *mut RawResult) -> c_int;
    pub fn sassy_hip_min_costs_reads(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                     reads: *const RawReads, k: usize, flags: u32, out_cost: *mut u8, out_strand: *mut u8) -> c_int;
    pub fn sassy_hip_best_pattern_reads(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                        reads: *const RawReads, k: usize, flags: u32, out_cost: *mut u8, out_pattern: *mut u32,
                                        out_strand: *mut u8) -> c_int;
    pub fn sassy_hip_best_matches_reads(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                                        reads: *const RawReads, k: usize, flags: u32, out: *mut *mut RawResult) -> c_int;
    pub fn sassy_hip_reads_relayout(reads: *const RawReads, first: u64, count: u64, dst_starts: *const u64, total: u64, pad: u8,
                                    d_dst: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
    // paired-end overlap: read r of r1 against the reverse complement of read r of r2, `out` holds sassy_hip_reads_n(r1) records
    pub fn sassy_hip_read_overlaps(s: *mut RawSearcher, r1: *const RawReads, r2: *const RawReads, min_overlap: u32, k: usize,
                                   max_permille: u32, flags: u32, out: *mut ReadOverlap) -> c_int;
    /// every pair with an accepted overlap merged into a new resident batch (one record per pair; free it with sassy_hip_reads_free)
    pub fn sassy_hip_merge_pairs(s: *mut RawSearcher, r1: *const RawReads, r2: *const RawReads, min_overlap: u32, k: usize,
                                 max_permille: u32, flags: u32, out_overlaps: *mut ReadOverlap, out_merged: *mut *mut RawReads) -> c_int;
    /// the 3' adapter and the low-quality tail cut off every read, into a new resident batch (one record per read)
    pub fn sassy_hip_trim_reads(s: *mut RawSearcher, reads: *const RawReads, adapters: *const *const u8, adapter_lens: *const usize,
                                n_adapters: usize, min_overlap: u32, k: usize, max_permille: u32, quality_cutoff: u32, min_length: u32,
                                flags: u32, out_trims: *mut ReadTrim, out_trimmed: *mut *mut RawReads) -> c_int;
    /// bytes [begins[r], begins[r] + lens[r]) of every read as a new resident batch
    pub fn sassy_hip_reads_slice(reads: *const RawReads, begins: *const u64, lens: *const u64, hip_stream: *mut std::ffi::c_void,
                                 out: *mut *mut RawReads) -> c_int;
    /// record j = bytes [begins[j], begins[j] + lens[j]) of read src[j] (begins, lens null: whole reads) as a new resident batch
    pub fn sassy_hip_reads_select(reads: *const RawReads, src: *const u64, begins: *const u64, lens: *const u64, n_out: u64,
                                  hip_stream: *mut std::ffi::c_void, out: *mut *mut RawReads) -> c_int;
    /// every read given to the sample whose barcode stands at a fixed place of one of its ends; a new resident batch sorted by sample
    pub fn sassy_hip_demux_reads(s: *mut RawSearcher, reads: *const RawReads, barcodes: *const *const u8, barcode_len: usize,
                                 n_barcodes: usize, at: u32, k: usize, min_delta: u32, flags: u32, out_assign: *mut ReadDemux,
                                 out_order: *mut u64, out_bounds: *mut u64, out_sorted: *mut *mut RawReads) -> c_int;
    /// sassy_hip_umi_groups over a window of every read of a resident batch: the four columns per read, mapped back
    pub fn sassy_hip_umi_groups_reads(s: *mut RawSearcher, reads: *const RawReads, at: u32, m: usize, k: usize, method: u32, flags: u32,
                                      out_label: *mut u32, out_size: *mut u32, out_rep: *mut u32, out_count: *mut u32, n_unique: *mut usize,
                                      n_groups: *mut usize) -> c_int;
    /// ... and of every group the read with the highest score kept, as a new resident batch (out_kept: which reads those are)
    pub fn sassy_hip_dedup_reads(s: *mut RawSearcher, reads: *const RawReads, at: u32, m: usize, k: usize, method: u32, flags: u32,
                                 out_label: *mut u32, out_size: *mut u32, out_rep: *mut u32, out_count: *mut u32, out_kept: *mut u64,
                                 n_unique: *mut usize, n_groups: *mut usize, out_dedup: *mut *mut RawReads) -> c_int;
    fn sassy_hip_search_shard_begin(s: *mut RawSearcher, pattern: *const u8, pattern_len: usize, d_text: *const u8,
                                    halo_len: u64, shard_len: u64, global_offset: u64, total_len: u64, k: usize,
                                    flags: u32, out: *mut *mut RawTicket) -> c_int;
    fn sassy_hip_search_finish(s: *mut RawSearcher, t: *mut RawTicket, out: *mut *mut RawResult) -> c_int;
    fn sassy_hip_encode_patterns(s: *mut RawSearcher, patterns: *const u8, npat: usize, plen: usize) -> *mut RawEncoded;
    fn sassy_hip_encoded_free(e: *mut RawEncoded);
    fn sassy_hip_search_encoded(s: *mut RawSearcher, e: *const RawEncoded, text: *const u8, text_len: usize,
                                k: usize, flags: u32, out: *mut *mut RawResult) -> c_int;
    // best-cost search (include/sassy_hip.h): one cost per (pattern, text) pair / the best pattern per text, no records
    fn sassy_hip_min_costs(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                           texts: *const *const u8, text_lens: *const usize, n_texts: usize, k: usize, flags: u32,
                           out_cost: *mut u8, out_strand: *mut u8) -> c_int;
    fn sassy_hip_best_pattern(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                              texts: *const *const u8, text_lens: *const usize, n_texts: usize, k: usize, flags: u32,
                              out_cost: *mut u8, out_pattern: *mut u32, out_strand: *mut u8) -> c_int;
    // best matches (include/sassy_hip.h): per text the one best match as a complete record
    fn sassy_hip_best_matches(s: *mut RawSearcher, patterns: *const *const u8, pattern_lens: *const usize, n_patterns: usize,
                              texts: *const *const u8, text_lens: *const usize, n_texts: usize, k: usize, flags: u32,
                              out: *mut *mut RawResult) -> c_int;
    fn sassy_hip_result_len(r: *const RawResult) -> usize;
    fn sassy_hip_result_matches(r: *const RawResult) -> *const RawMatch;
    fn sassy_hip_result_cigars(r: *const RawResult) -> *const c_char;
    fn sassy_hip_result_free(r: *mut RawResult);
    fn sassy_hip_set_only_best_match(s: *mut RawSearcher, on: c_int) -> c_int;
    fn sassy_hip_set_max_n_frac(s: *mut RawSearcher, f: f32) -> c_int;
    fn sassy_hip_set_device(s: *mut RawSearcher, device: c_int) -> c_int;
    fn sassy_hip_merge_shards(results: *const *const RawResult, n: usize, incoming_state: c_int,
                              out: *mut *mut RawResult) -> c_int;
    fn sassy_hip_multi_new(alphabet: *const c_char, alpha: f32, devices: *const c_int, n_devices: usize) -> *mut RawMulti;
    fn sassy_hip_multi_set_text(m: *mut RawMulti, text: *const u8, len: usize, max_pattern_len: usize, max_k: usize) -> c_int;
    fn sassy_hip_multi_search(m: *mut RawMulti, pattern: *const u8, pattern_len: usize, k: usize, flags: u32,
                              out: *mut *mut RawResult) -> c_int;
    fn sassy_hip_multi_free(m: *mut RawMulti);
    // searches in flight over several devices (include/sassy_hip.h)
    fn sassy_hip_multi_set_pipe_depth(m: *mut RawMulti, depth: c_int) -> c_int;
    fn sassy_hip_multi_search_begin(m: *mut RawMulti, pattern: *const u8, pattern_len: usize, k: usize, flags: u32,
                                    out: *mut *mut RawMultiTicket) -> c_int;
    fn sassy_hip_multi_search_finish(m: *mut RawMulti, ticket: *mut RawMultiTicket, out: *mut *mut RawResult) -> c_int;
}

#[repr(C)]
pub struct RawMulti {
    _p: [u8; 0],
}

/// One text over several GPUs inside one process (include/sassy_hip.h: sassy_hip_multi_*): the reference's thread
/// fan-out (bin/grep.rs:476-503) with a device per thread.  Forward strand, like the shard calls.
pub struct MultiSearcher {
    raw: *mut RawMulti,
}

impl MultiSearcher {
    /// `devices`: empty = every visible device.
    pub fn new(alphabet: &str, devices: &[i32]) -> Self {
        let a = std::ffi::CString::new(alphabet).unwrap();
        let raw = unsafe { sassy_hip_multi_new(a.as_ptr(), f32::NAN, if devices.is_empty() { std::ptr::null() } else { devices.as_ptr() }, devices.len()) };
        assert!(!raw.is_null(), "{}", last_error());
        MultiSearcher { raw }
    }
    pub fn set_text(&mut self, text: &[u8], max_pattern_len: usize, max_k: usize) {
        let rc = unsafe { sassy_hip_multi_set_text(self.raw, text.as_ptr(), text.len(), max_pattern_len, max_k) };
        assert_eq!(rc, 0, "{}", last_error());
    }
    pub fn search(&mut self, pattern: &[u8], k: usize) -> Vec<Match> {
        let mut res = std::ptr::null_mut();
        let rc = unsafe { sassy_hip_multi_search(self.raw, pattern.as_ptr(), pattern.len(), k, 0, &mut res) };
        assert_eq!(rc, 0, "{}", last_error());
        unsafe { collect(res) }
    }
}

impl Drop for MultiSearcher {
    fn drop(&mut self) {
        unsafe { sassy_hip_multi_free(self.raw) }
    }
}

/// The reference's `Strand` (src/search.rs:107-119).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Strand {
    Fwd,
    Rc,
}

/// The reference's `Match` (src/search.rs:35-62); `cigar` in SAM text form (`pa_types::Cigar::to_string`).
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct Match {
    pub pattern_idx: usize,
    pub text_idx: usize,
    pub text_start: usize,
    pub text_end: usize,
    pub pattern_start: usize,
    pub pattern_end: usize,
    pub cost: i32,
    pub strand: Strand,
    pub cigar: String,
}

/// Alphabet marker types, as the reference's `profiles::{Dna, Iupac, Ascii}`.
pub trait Profile {
    const NAME: &'static str;
}
pub struct Dna;
pub struct Iupac;
pub struct Ascii;
impl Profile for Dna {
    const NAME: &'static str = "dna";
}
impl Profile for Iupac {
    const NAME: &'static str = "iupac";
}
impl Profile for Ascii {
    const NAME: &'static str = "ascii";
}

pub struct Searcher<P: Profile> {
    raw: *mut RawSearcher,
    _p: PhantomData<P>,
}

/// `EncodedPatterns<P>` (src/pattern_tiling/general.rs:132-150): opaque on both sides.
pub struct EncodedPatterns<P: Profile> {
    raw: *mut RawEncoded,
    _p: PhantomData<P>,
}
impl<P: Profile> Drop for EncodedPatterns<P> {
    fn drop(&mut self) {
        unsafe { sassy_hip_encoded_free(self.raw) }
    }
}

/// A search in flight (`include/sassy_hip.h`: sassy_hip_search_shard_begin).
pub struct Ticket(*mut RawTicket);

fn last_error() -> String {
    unsafe { CStr::from_ptr(sassy_hip_last_error()) }.to_string_lossy().into_owned()
}

unsafe fn collect(res: *mut RawResult) -> Vec<Match> {
    let n = sassy_hip_result_len(res);
    let rows = std::slice::from_raw_parts(sassy_hip_result_matches(res), n);
    let pool = sassy_hip_result_cigars(res);
    let out = rows
        .iter()
        .map(|m| Match {
            pattern_idx: m.pattern_idx as usize,
            text_idx: m.text_idx as usize,
            text_start: m.text_start as usize,
            text_end: m.text_end as usize,
            pattern_start: m.pattern_start as usize,
            pattern_end: m.pattern_end as usize,
            cost: m.cost,
            strand: if m.strand == 0 { Strand::Fwd } else { Strand::Rc },
            cigar: CStr::from_ptr(pool.add(m.cigar_off as usize)).to_string_lossy().into_owned(),
        })
        .collect();
    sassy_hip_result_free(res);
    out
}

impl<P: Profile> Searcher<P> {
    /// `Searcher::new(rc, alpha)` (src/search.rs:486-503); panics like the reference on an invalid combination.
    pub fn new(rc: bool, alpha: Option<f32>) -> Self {
        let name = CString::new(P::NAME).unwrap();
        let raw = unsafe { sassy_hip_searcher_new(name.as_ptr(), rc, alpha.unwrap_or(f32::NAN)) };
        assert!(!raw.is_null(), "{}", last_error());
        Searcher { raw, _p: PhantomData }
    }
    /// `Searcher::new_fwd()` / `new_rc()` (src/search.rs:261-283).
    pub fn new_fwd() -> Self {
        Self::new(false, None)
    }
    pub fn new_rc() -> Self {
        Self::new(true, None)
    }
    pub fn only_best_match(self) -> Self {
        unsafe { sassy_hip_set_only_best_match(self.raw, 1) };
        self
    }
    pub fn with_max_n_frac(self, f: f32) -> Self {
        unsafe { sassy_hip_set_max_n_frac(self.raw, f) };
        self
    }

    fn run(&mut self, pattern: &[u8], text: &[u8], k: usize, flags: u32) -> Vec<Match> {
        let mut res = std::ptr::null_mut();
        let rc = unsafe {
            sassy_hip_search(self.raw, pattern.as_ptr(), pattern.len(), text.as_ptr(), text.len(), k, flags, &mut res)
        };
        assert_eq!(rc, 0, "{}", last_error()); // the reference panics on its errors
        unsafe { collect(res) }
    }
    /// `Searcher::search` (src/search.rs:510-525): rightmost local minima with cost <= k.
    pub fn search(&mut self, pattern: &[u8], text: &[u8], k: usize) -> Vec<Match> {
        self.run(pattern, text, k, 0)
    }
    /// `Searcher::search_all` (src/search.rs:685-700).
    pub fn search_all(&mut self, pattern: &[u8], text: &[u8], k: usize) -> Vec<Match> {
        self.run(pattern, text, k, ALL_MINIMA)
    }
    /// `Searcher::encode_patterns` (src/search.rs:404-406): equal-length patterns (<= 64).
    pub fn encode_patterns(&mut self, patterns: &[Vec<u8>]) -> EncodedPatterns<P> {
        assert!(!patterns.is_empty(), "No queries provided");
        let plen = patterns[0].len();
        assert!(patterns.iter().all(|p| p.len() == plen), "All pattern must have the same length");
        let flat: Vec<u8> = patterns.iter().flatten().copied().collect();
        let raw = unsafe { sassy_hip_encode_patterns(self.raw, flat.as_ptr(), patterns.len(), plen) };
        assert!(!raw.is_null(), "{}", last_error());
        EncodedPatterns { raw, _p: PhantomData }
    }
    /// `Searcher::search_encoded_patterns` (src/search.rs:415-423); owned `Vec` instead of a borrowed slice.
    pub fn search_encoded_patterns(&mut self, encoded: &EncodedPatterns<P>, text: &[u8], k: usize) -> Vec<Match> {
        let mut res = std::ptr::null_mut();
        let rc = unsafe { sassy_hip_search_encoded(self.raw, encoded.raw, text.as_ptr(), text.len(), k, 0, &mut res) };
        assert_eq!(rc, 0, "{}", last_error());
        unsafe { collect(res) }
    }

    /// The smallest cost of any match of pattern p in text t, row-major `[p * texts.len() + t]`, `NO_MATCH` where there is
    /// none of cost <= k (what `only_best_match().without_trace()` under `search_many` gives per pair, reduced).
    pub fn min_costs(&mut self, patterns: &[&[u8]], texts: &[&[u8]], k: usize) -> Vec<u8> {
        let (pp, pl): (Vec<*const u8>, Vec<usize>) = patterns.iter().map(|p| (p.as_ptr(), p.len())).unzip();
        let (tp, tl): (Vec<*const u8>, Vec<usize>) = texts.iter().map(|t| (t.as_ptr(), t.len())).unzip();
        let mut cost = vec![NO_MATCH; patterns.len() * texts.len()];
        let rc = unsafe {
            sassy_hip_min_costs(self.raw, pp.as_ptr(), pl.as_ptr(), pp.len(), tp.as_ptr(), tl.as_ptr(), tp.len(), k, 0,
                                cost.as_mut_ptr(), std::ptr::null_mut())
        };
        assert_eq!(rc, 0, "{}", last_error());
        cost
    }

    /// Per text: (cost, pattern, strand) of the best pattern -- lowest cost, then lowest index, then Fwd; cost `NO_MATCH` and
    /// pattern `u32::MAX` where no pattern matches with cost <= k.
    pub fn best_pattern(&mut self, patterns: &[&[u8]], texts: &[&[u8]], k: usize) -> Vec<(u8, u32, Strand)> {
        let (pp, pl): (Vec<*const u8>, Vec<usize>) = patterns.iter().map(|p| (p.as_ptr(), p.len())).unzip();
        let (tp, tl): (Vec<*const u8>, Vec<usize>) = texts.iter().map(|t| (t.as_ptr(), t.len())).unzip();
        let (mut cost, mut pat, mut strand) = (vec![NO_MATCH; texts.len()], vec![u32::MAX; texts.len()], vec![0u8; texts.len()]);
        let rc = unsafe {
            sassy_hip_best_pattern(self.raw, pp.as_ptr(), pl.as_ptr(), pp.len(), tp.as_ptr(), tl.as_ptr(), tp.len(), k, 0,
                                   cost.as_mut_ptr(), pat.as_mut_ptr(), strand.as_mut_ptr())
        };
        assert_eq!(rc, 0, "{}", last_error());
        (0..texts.len()).map(|t| (cost[t], pat[t], if strand[t] != 0 { Strand::Rc } else { Strand::Fwd })).collect()
    }

    /// Hamming search over a batch of texts: every start with at most `k` mismatches of every pattern in every text, ordered
    /// by (pattern_idx, Fwd before Rc, text_idx, text_start); coordinates are relative to the record's text.
    pub fn search_hamming_many(&mut self, patterns: &[&[u8]], texts: &[&[u8]], k: usize) -> Vec<Match> {
        let (pp, pl): (Vec<*const u8>, Vec<usize>) = patterns.iter().map(|p| (p.as_ptr(), p.len())).unzip();
        let (tp, tl): (Vec<*const u8>, Vec<usize>) = texts.iter().map(|t| (t.as_ptr(), t.len())).unzip();
        let mut res = std::ptr::null_mut();
        let rc = unsafe {
            sassy_hip_search_hamming_many(self.raw, pp.as_ptr(), pl.as_ptr(), pp.len(), tp.as_ptr(), tl.as_ptr(), tp.len(), k, 0, &mut res)
        };
        assert_eq!(rc, 0, "{}", last_error());
        unsafe { collect(res) }
    }

    /// Per text the best Hamming hit over all patterns and strands: (cost, pattern, strand, start) -- lowest cost, then
    /// lowest pattern index, then Fwd before Rc, then the leftmost start; (`NO_MATCH`, `u32::MAX`, Fwd, `u64::MAX`) where no
    /// pattern has a hit with at most `k` mismatches.
    pub fn hamming_best_pattern(&mut self, patterns: &[&[u8]], texts: &[&[u8]], k: usize) -> Vec<(u8, u32, Strand, u64)> {
        let (pp, pl): (Vec<*const u8>, Vec<usize>) = patterns.iter().map(|p| (p.as_ptr(), p.len())).unzip();
        let (tp, tl): (Vec<*const u8>, Vec<usize>) = texts.iter().map(|t| (t.as_ptr(), t.len())).unzip();
        let n = texts.len();
        let (mut cost, mut pat, mut strand, mut start) = (vec![NO_MATCH; n], vec![u32::MAX; n], vec![0u8; n], vec![u64::MAX; n]);
        let rc = unsafe {
            sassy_hip_hamming_best_pattern(self.raw, pp.as_ptr(), pl.as_ptr(), pp.len(), tp.as_ptr(), tl.as_ptr(), tp.len(), k, 0,
                                           cost.as_mut_ptr(), pat.as_mut_ptr(), strand.as_mut_ptr(), start.as_mut_ptr())
        };
        assert_eq!(rc, 0, "{}", last_error());
        (0..n).map(|t| (cost[t], pat[t], if strand[t] != 0 { Strand::Rc } else { Strand::Fwd }, start[t])).collect()
    }

    /// Hamming hit counts of one host text: `[(2 p + strand) (k + 1) + c]` = the number of hits of pattern `p` on that strand
    /// (0 Fwd, 1 Rc) with exactly `c` mismatches -- what `search_hamming` would list, counted on the device.  `k <= 254`.
    pub fn hamming_counts(&mut self, patterns: &[&[u8]], text: &[u8], k: usize) -> Vec<u64> {
        let (pp, pl): (Vec<*const u8>, Vec<usize>) = patterns.iter().map(|p| (p.as_ptr(), p.len())).unzip();
        let mut counts = vec![0u64; patterns.len() * 2 * (k + 1)];
        let rc = unsafe {
            sassy_hip_hamming_counts(self.raw, pp.as_ptr(), pl.as_ptr(), pp.len(), text.as_ptr(), text.len(), k, 0, counts.as_mut_ptr())
        };
        assert_eq!(rc, 0, "{}", last_error());
        counts
    }

    /// `hamming_counts` over a batch of texts, summed over all of them (the records of `search_hamming_many`, counted).
    pub fn hamming_counts_many(&mut self, patterns: &[&[u8]], texts: &[&[u8]], k: usize) -> Vec<u64> {
        let (pp, pl): (Vec<*const u8>, Vec<usize>) = patterns.iter().map(|p| (p.as_ptr(), p.len())).unzip();
        let (tp, tl): (Vec<*const u8>, Vec<usize>) = texts.iter().map(|t| (t.as_ptr(), t.len())).unzip();
        let mut counts = vec![0u64; patterns.len() * 2 * (k + 1)];
        let rc = unsafe {
            sassy_hip_hamming_counts_many(self.raw, pp.as_ptr(), pl.as_ptr(), pp.len(), tp.as_ptr(), tl.as_ptr(), tp.len(), k, 0,
                                          counts.as_mut_ptr())
        };
        assert_eq!(rc, 0, "{}", last_error());
        counts
    }

    /// The products of primer pairs `(fwd, rev)`, both written 5'->3', in one host text (in-silico PCR): every `(strand,
    /// start, end)` with `min_len <= end - start <= max_len` whose two primer sites have at most `k` mismatches each, ordered
    /// by `(pair_idx, strand, start, end)`; joined on the device.  `k <= 254`, `max_len <= 2^24`, Dna and Iupac searchers.
    pub fn hamming_amplicons(&mut self, pairs: &[(&[u8], &[u8])], text: &[u8], k: usize, min_len: u64, max_len: u64) -> Vec<Amplicon> {
        let (fp, fl): (Vec<*const u8>, Vec<usize>) = pairs.iter().map(|p| (p.0.as_ptr(), p.0.len())).unzip();
        let (rp, rl): (Vec<*const u8>, Vec<usize>) = pairs.iter().map(|p| (p.1.as_ptr(), p.1.len())).unzip();
        let mut out: *mut Amplicon = std::ptr::null_mut();
        let mut n = 0usize;
        let rc = unsafe {
            sassy_hip_hamming_amplicons(self.raw, fp.as_ptr(), fl.as_ptr(), rp.as_ptr(), rl.as_ptr(), pairs.len(), text.as_ptr(), text.len(),
                                        k, min_len, max_len, 0, &mut out, &mut n)
        };
        assert_eq!(rc, 0, "{}", last_error());
        let v = if n == 0 { Vec::new() } else { unsafe { std::slice::from_raw_parts(out, n) }.to_vec() };
        unsafe { sassy_hip_amplicons_free(out) };
        v
    }

    /// All-vs-all Hamming distances between two lists of sequences of `m` bytes each, stored back to back: every `(a_idx,
    /// b_idx, strand)` with at most `k` mismatches, ordered by `(a_idx, b_idx, strand)`.  `b = None`: `a` against itself, every
    /// unordered pair once (strand 0: `a_idx < b_idx`; strand 1: `a_idx <= b_idx`).  `m <= 128`, `k <= 254`.
    pub fn hamming_pairs(&mut self, a: &[u8], b: Option<&[u8]>, m: usize, k: usize) -> Vec<HammingPair> {
        assert!(m > 0 && a.len() % m == 0 && b.map_or(true, |b| b.len() % m == 0), "lists hold whole sequences of m bytes");
        let (bp, nb) = b.map_or((std::ptr::null(), 0), |b| (b.as_ptr(), b.len() / m));
        let mut out: *mut HammingPair = std::ptr::null_mut();
        let mut n = 0usize;
        let rc = unsafe { sassy_hip_hamming_pairs(self.raw, a.as_ptr(), a.len() / m, bp, nb, m, k, 0, &mut out, &mut n) };
        assert_eq!(rc, 0, "{}", last_error());
        let v = if n == 0 { Vec::new() } else { unsafe { std::slice::from_raw_parts(out, n) }.to_vec() };
        unsafe { sassy_hip_hamming_pairs_free(out) };
        v
    }

    /// Per sequence of `a` its nearest sequence of `b` within `k` mismatches: `(cost, index, strand, ties)` -- the smallest
    /// under `(cost, index, Fwd before Rc)` and how many candidates share that cost; `(NO_MATCH, u32::MAX, Fwd, 0)` where there
    /// is none.  `b = None`: the nearest other sequence of `a` (only `(index == i, Fwd)` is no candidate).
    pub fn hamming_nearest(&mut self, a: &[u8], b: Option<&[u8]>, m: usize, k: usize) -> Vec<(u8, u32, Strand, u32)> {
        assert!(m > 0 && a.len() % m == 0 && b.map_or(true, |b| b.len() % m == 0), "lists hold whole sequences of m bytes");
        let (bp, nb) = b.map_or((std::ptr::null(), 0), |b| (b.as_ptr(), b.len() / m));
        let n = a.len() / m;
        let (mut cost, mut index, mut strand, mut ties) = (vec![0u8; n], vec![0u32; n], vec![0u8; n], vec![0u32; n]);
        let rc = unsafe {
            sassy_hip_hamming_nearest(self.raw, a.as_ptr(), n, bp, nb, m, k, 0, cost.as_mut_ptr(), index.as_mut_ptr(), strand.as_mut_ptr(),
                                      ties.as_mut_ptr())
        };
        assert_eq!(rc, 0, "{}", last_error());
        (0..n).map(|i| (cost[i], index[i], if strand[i] != 0 { Strand::Rc } else { Strand::Fwd }, ties[i])).collect()
    }

    /// All-vs-all edit (Levenshtein) distances: `hamming_pairs` with substitutions, insertions and deletions at 1 each, both
    /// sequences consumed whole.  `a` holds sequences of `m_a` bytes, `b` of `m_b` bytes (`(list, m_b)`), both `<= 64`;
    /// `b = None`: `a` against itself.  Records and order as `hamming_pairs`; `cost` is the edit distance.  `k <= 254`.
    pub fn edit_pairs(&mut self, a: &[u8], m_a: usize, b: Option<(&[u8], usize)>, k: usize) -> Vec<HammingPair> {
        assert!(m_a > 0 && a.len() % m_a == 0 && b.map_or(true, |(b, m_b)| m_b > 0 && b.len() % m_b == 0), "lists hold whole sequences");
        let (bp, nb, m_b) = b.map_or((std::ptr::null(), 0, 0), |(b, m_b)| (b.as_ptr(), b.len() / m_b, m_b));
        let mut out: *mut HammingPair = std::ptr::null_mut();
        let mut n = 0usize;
        let rc = unsafe { sassy_hip_edit_pairs(self.raw, a.as_ptr(), a.len() / m_a, m_a, bp, nb, m_b, k, 0, &mut out, &mut n) };
        assert_eq!(rc, 0, "{}", last_error());
        let v = if n == 0 { Vec::new() } else { unsafe { std::slice::from_raw_parts(out, n) }.to_vec() };
        unsafe { sassy_hip_edit_pairs_free(out) };
        v
    }

    /// Per sequence of `a` its nearest sequence of `b` within `k` edits: `(cost, index, strand, ties)` as `hamming_nearest`
    /// gives them.  Lists as for `edit_pairs`.
    pub fn edit_nearest(&mut self, a: &[u8], m_a: usize, b: Option<(&[u8], usize)>, k: usize) -> Vec<(u8, u32, Strand, u32)> {
        assert!(m_a > 0 && a.len() % m_a == 0 && b.map_or(true, |(b, m_b)| m_b > 0 && b.len() % m_b == 0), "lists hold whole sequences");
        let (bp, nb, m_b) = b.map_or((std::ptr::null(), 0, 0), |(b, m_b)| (b.as_ptr(), b.len() / m_b, m_b));
        let n = a.len() / m_a;
        let (mut cost, mut index, mut strand, mut ties) = (vec![0u8; n], vec![0u32; n], vec![0u8; n], vec![0u32; n]);
        let rc = unsafe {
            sassy_hip_edit_nearest(self.raw, a.as_ptr(), n, m_a, bp, nb, m_b, k, 0, cost.as_mut_ptr(), index.as_mut_ptr(), strand.as_mut_ptr(),
                                   ties.as_mut_ptr())
        };
        assert_eq!(rc, 0, "{}", last_error());
        (0..n).map(|i| (cost[i], index[i], if strand[i] != 0 { Strand::Rc } else { Strand::Fwd }, ties[i])).collect()
    }

    /// The groups the sequences of `a` (`m` bytes each, `m <= 128`) form: the connected components of the graph that joins
    /// two sequences within `k` mismatches of each other (an rc searcher: or of each other's reverse complement).
    /// `(labels, sizes, n_clusters)`: `labels[i]` is the smallest index of `i`'s component, `sizes[i]` its size.  `k <= 254`.
    pub fn hamming_clusters(&mut self, a: &[u8], m: usize, k: usize) -> (Vec<u32>, Vec<u32>, usize) {
        assert!(m > 0 && a.len() % m == 0, "the list holds whole sequences of m bytes");
        let n = a.len() / m;
        let (mut labels, mut sizes, mut count) = (vec![0u32; n], vec![0u32; n], 0usize);
        let rc = unsafe { sassy_hip_hamming_clusters(self.raw, a.as_ptr(), n, m, k, 0, labels.as_mut_ptr(), sizes.as_mut_ptr(), &mut count) };
        assert_eq!(rc, 0, "{}", last_error());
        (labels, sizes, count)
    }

    /// `hamming_clusters` under the edit distance: an edge where at most `k` substitutions, insertions and deletions turn one
    /// sequence into the other.  `m <= 64`.
    pub fn edit_clusters(&mut self, a: &[u8], m: usize, k: usize) -> (Vec<u32>, Vec<u32>, usize) {
        assert!(m > 0 && a.len() % m == 0, "the list holds whole sequences of m bytes");
        let n = a.len() / m;
        let (mut labels, mut sizes, mut count) = (vec![0u32; n], vec![0u32; n], 0usize);
        let rc = unsafe { sassy_hip_edit_clusters(self.raw, a.as_ptr(), n, m, k, 0, labels.as_mut_ptr(), sizes.as_mut_ptr(), &mut count) };
        assert_eq!(rc, 0, "{}", last_error());
        (labels, sizes, count)
    }

    /// UMI grouping of the sequences of `a` (`m` bytes each, `m <= 128`): identical reads collapsed, the distinct sequences
    /// grouped by `method` -- 0 unique (collapse only), 1 cluster (connected components within `k` mismatches), 2 directional
    /// (a neighbour of count `c_u >= 2 c_v - 1` absorbs `v`; UMI-tools' rule with the tie order fixed).
    /// `(labels, sizes, reps, counts, n_unique, n_groups)`: `reps[i]` is the first duplicate of `i`, `counts[i]` the number
    /// of its duplicates, `labels[i]` the first index of its group's opener, `sizes[i]` the reads of that group.  `k <= 254`.
    pub fn umi_groups(&mut self, a: &[u8], m: usize, k: usize, method: u32) -> (Vec<u32>, Vec<u32>, Vec<u32>, Vec<u32>, usize, usize) {
        assert!(m > 0 && a.len() % m == 0, "the list holds whole sequences of m bytes");
        let n = a.len() / m;
        let (mut labels, mut sizes, mut reps, mut counts) = (vec![0u32; n], vec![0u32; n], vec![0u32; n], vec![0u32; n]);
        let (mut n_unique, mut n_groups) = (0usize, 0usize);
        let rc = unsafe {
            sassy_hip_umi_groups(self.raw, a.as_ptr(), n, m, k, method, 0, labels.as_mut_ptr(), sizes.as_mut_ptr(), reps.as_mut_ptr(),
                                 counts.as_mut_ptr(), &mut n_unique, &mut n_groups)
        };
        assert_eq!(rc, 0, "{}", last_error());
        (labels, sizes, reps, counts, n_unique, n_groups)
    }

    /// Per text the one best match over all patterns and strands as a complete record: lowest cost, then lowest pattern
    /// index, then Fwd before Rc, then the rightmost end in the strand's scan direction (the reference's `only_best_match`
    /// rule, src/search.rs:1392-1412).  At most one `Match` per text, in ascending `text_idx`.
    pub fn best_matches(&mut self, patterns: &[&[u8]], texts: &[&[u8]], k: usize) -> Vec<Match> {
        let (pp, pl): (Vec<*const u8>, Vec<usize>) = patterns.iter().map(|p| (p.as_ptr(), p.len())).unzip();
        let (tp, tl): (Vec<*const u8>, Vec<usize>) = texts.iter().map(|t| (t.as_ptr(), t.len())).unzip();
        let mut res = std::ptr::null_mut();
        let rc = unsafe {
            sassy_hip_best_matches(self.raw, pp.as_ptr(), pl.as_ptr(), pp.len(), tp.as_ptr(), tl.as_ptr(), tp.len(), k, 0, &mut res)
        };
        assert_eq!(rc, 0, "{}", last_error());
        unsafe { collect(res) }
    }

    /// A stream of searches over a text that lives in HBM: queue one and go on (up to two in flight).
    ///
    /// # Safety
    /// `d_text` must be a device pointer to `total_len` resident bytes that stay unchanged until `finish`.
    pub unsafe fn begin_on_device(&mut self, pattern: &[u8], d_text: *const u8, total_len: u64, k: usize) -> Ticket {
        let mut t = std::ptr::null_mut();
        let rc = sassy_hip_search_shard_begin(self.raw, pattern.as_ptr(), pattern.len(), d_text, 0, total_len, 0, total_len,
                                              k, 0, &mut t);
        assert_eq!(rc, 0, "{}", last_error());
        Ticket(t)
    }
    pub fn finish(&mut self, ticket: Ticket) -> Vec<Match> {
        let mut res = std::ptr::null_mut();
        let rc = unsafe { sassy_hip_search_finish(self.raw, ticket.0, &mut res) };
        assert_eq!(rc, 0, "{}", last_error());
        unsafe { collect(res) }
    }
}

impl<P: Profile> Drop for Searcher<P> {
    fn drop(&mut self) {
        unsafe { sassy_searcher_free(self.raw) }
    }
}
