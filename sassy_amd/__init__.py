"""sassy_amd -- MI355X-native drop-in for sassy's bit-parallel search path.

The product is ``sassy_amd/lib/libsassy_hip.so`` (hand-written HIP for gfx950 behind the C-ABI of
``include/sassy.h`` / ``include/sassy_hip.h``).  This package is the thin Python host mirror of
the reference's Python / Rust searcher interface for that path:

    reference (src/python.rs:26-220)            here
    sassy.Searcher(alphabet, rc, alpha)     ->  sassy_amd.Searcher(alphabet, rc, alpha)
    .search(pattern, text, k)               ->  .search(pattern, text, k)
    .search_all(pattern, text, k)           ->  .search_all(pattern, text, k)
    Searcher::encode_patterns / search_encoded_patterns (src/search.rs:404-423)
                                            ->  .encode_patterns(...) / .search_encoded_patterns(...)
    Match getters pattern_idx, text_start, text_end, pattern_start, pattern_end, cost,
    strand ('+'/'-'), cigar                 ->  the same attribute names

There is no CPU implementation in here: without the compiled library or without a HIP device
every search raises ``SassyHipError``.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from collections.abc import Sequence as _SequenceABC
from typing import List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "lib", "libsassy_hip.so")
if os.environ.get("SASSY_HIP_LIBRARY"):  # A/B timing of two builds on one box (tools only)
    _SO = os.environ["SASSY_HIP_LIBRARY"]

ALL_MINIMA = 1
WITHOUT_TRACE = 2
TEXT_ON_DEVICE = 4
NO_MATCH = 255  # min_costs / best_pattern: no match of cost <= k
TEXT_UNCHANGED = 8
CLASS_MAX_CUBES = 256  # SASSY_HIP_CLASS_MAX_CUBES: cubes of one class pattern, all distinct sets together
LINE_SPANS = 16  # sassy_hip_search only: resolve the matches to their lines (Result.line_spans)
KEEP_QUALITY = 32  # sassy_hip_fastq_parse only: the handle keeps the base qualities on the device (DeviceReads(keep_quality=True))
UINT64_MAX = (1 << 64) - 1
UMI_METHODS = {"unique": 0, "cluster": 1, "directional": 2}  # SASSY_HIP_UMI_*: Searcher.umi_groups


class SassyHipError(RuntimeError):
    pass


class CMatch(C.Structure):
    """include/sassy.h: sassy_Match (40 bytes, align 8)."""
    _fields_ = [
        ("text_start", C.c_size_t),
        ("text_end", C.c_size_t),
        ("pattern_start", C.c_size_t),
        ("pattern_end", C.c_size_t),
        ("cost", C.c_int32),
        ("strand", C.c_uint8),
    ]


class _HipMatch(C.Structure):
    _fields_ = [
        ("pattern_idx", C.c_uint64),
        ("text_idx", C.c_uint64),
        ("text_start", C.c_uint64),
        ("text_end", C.c_uint64),
        ("pattern_start", C.c_uint64),
        ("pattern_end", C.c_uint64),
        ("cost", C.c_int32),
        ("strand", C.c_uint8),
        ("pad_", C.c_uint8 * 3),
        ("cigar_off", C.c_uint32),
        ("cigar_len", C.c_uint32),
    ]


class LineSpan(C.Structure):
    """include/sassy_hip.h: sassy_hip_LineSpan (32 bytes)."""
    _fields_ = [
        ("line_no", C.c_uint64),
        ("last_line_no", C.c_uint64),
        ("line_start", C.c_uint64),
        ("line_end", C.c_uint64),
    ]


# int fn(pattern, pattern_len, text_till_end, end_pos, strand, user)  (include/sassy_hip.h)
END_FILTER = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, C.c_int,
                         C.c_void_p)


class Stats(C.Structure):
    _fields_ = [
        ("scan_ms", C.c_double),
        ("trace_ms", C.c_double),
        ("total_ms", C.c_double),
        ("text_bytes", C.c_uint64),
        ("scan_launches", C.c_uint64),
        ("candidates", C.c_uint64),
        ("cond_resolved", C.c_uint64),
        ("chunks", C.c_uint64),
        ("blocks", C.c_uint64),
        ("word_rows", C.c_uint64),
        ("blocks_per_chunk", C.c_uint32),
        ("warmup_blocks", C.c_uint32),
        ("grid", C.c_uint32),
        ("filtered", C.c_uint32),
        ("filter_ms", C.c_double),
        ("hit_blocks", C.c_uint64),
        ("piece_len", C.c_uint32),
        ("fused", C.c_uint32),
        ("host_enqueue_ms", C.c_double),
        ("host_wait_ms", C.c_double),
        ("host_post_ms", C.c_double),
        ("live_blocks", C.c_uint64),
        ("pair", C.c_uint32),
        ("pass_patterns", C.c_uint32),
        ("plane_launches", C.c_uint32),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "pad_"}


def option_table():
    """[(name, default, what it does)] of every switch of the library (csrc/switches.h)."""
    rows = []
    for line in lib().sassy_hip_option_table().decode().splitlines():
        name, dflt, doc = line.split("\t", 2)
        rows.append((name, dflt, doc))
    return rows


# every symbol include/sassy.h and include/sassy_hip.h declare
EXPORTED_SYMBOLS = [
    "sassy_searcher", "sassy_searcher_free", "search", "sassy_matches_free",
    "sassy_hip_last_error", "sassy_hip_version", "sassy_hip_device_count",
    "sassy_hip_searcher_new", "sassy_hip_set_stream", "sassy_hip_get_stats",
    "sassy_hip_search", "sassy_hip_search_all_alignments", "sassy_hip_search_shard", "sassy_hip_required_halo",
    "sassy_hip_search_shard_begin", "sassy_hip_search_finish", "sassy_hip_set_pipe_depth", "sassy_hip_set_geometry_tuner", "sassy_hip_set_reference_lanes",
    "sassy_hip_result_len", "sassy_hip_result_matches", "sassy_hip_result_cigars",
    "sassy_hip_result_cigars_len", "sassy_hip_pack_rows", "sassy_hip_enable_counters", "sassy_hip_set_timing",
    "sassy_hip_set_only_best_match", "sassy_hip_set_max_n_frac", "sassy_hip_search_with_fn",
    "sassy_hip_set_max_overhang", "sassy_hip_set_prefilter", "sassy_hip_set_fused",
    "sassy_hip_set_option", "sassy_hip_get_option", "sassy_hip_option_table", "sassy_hip_plant_phase",
    "sassy_hip_set_device", "sassy_hip_get_device", "sassy_hip_merge_shards",
    "sassy_hip_multi_new", "sassy_hip_multi_shards", "sassy_hip_multi_device", "sassy_hip_multi_searcher",
    "sassy_hip_multi_set_text", "sassy_hip_multi_generate_dna", "sassy_hip_multi_plant", "sassy_hip_multi_search",
    "sassy_hip_multi_free",
    "sassy_hip_search_many", "sassy_hip_min_costs", "sassy_hip_best_pattern", "sassy_hip_best_matches", "sassy_hip_tsv_header", "sassy_hip_format_tsv",
    "sassy_hip_result_exit_state", "sassy_hip_result_conditional_index", "sassy_hip_result_free",
    "sassy_hip_encode_patterns", "sassy_hip_encoded_free", "sassy_hip_search_encoded",
    "sassy_hip_multi_set_rc", "sassy_hip_multi_set_replicated", "sassy_hip_multi_search_encoded", "sassy_hip_multi_search_many",
    "sassy_hip_multi_set_pipe_depth", "sassy_hip_multi_search_begin", "sassy_hip_multi_search_finish", "sassy_hip_multi_layout", "sassy_hip_seed_layout", "sassy_hip_seed_test_rows",
    "sassy_hip_generate_dna", "sassy_hip_generate_genome_like", "sassy_hip_plant",
    "sassy_hip_malloc", "sassy_hip_free", "sassy_hip_memcpy_h2d", "sassy_hip_memcpy_d2h",
    "sassy_hip_line_spans", "sassy_hip_result_line_spans", "sassy_hip_line_tile", "sassy_hip_line_span_times",
    "sassy_hip_search_classes", "sassy_hip_class_cover",
    "sassy_hip_search_hamming", "sassy_hip_search_hamming_many", "sassy_hip_hamming_best_pattern",
    "sassy_hip_hamming_counts", "sassy_hip_hamming_counts_many",
    "sassy_hip_hamming_amplicons", "sassy_hip_amplicons_free",
    "sassy_hip_hamming_pairs", "sassy_hip_hamming_pairs_free", "sassy_hip_hamming_nearest",
    "sassy_hip_edit_pairs", "sassy_hip_edit_pairs_free", "sassy_hip_edit_nearest",
    "sassy_hip_hamming_clusters", "sassy_hip_edit_clusters", "sassy_hip_umi_groups",
    "sassy_hip_fasta_unwrap", "sassy_hip_fasta_n_records", "sassy_hip_fasta_records", "sassy_hip_fasta_text",
    "sassy_hip_fasta_text_bytes", "sassy_hip_fasta_free",
    "sassy_hip_fastq_parse", "sassy_hip_reads_n", "sassy_hip_reads_records", "sassy_hip_reads_text", "sassy_hip_reads_text_bytes",
    "sassy_hip_reads_longest", "sassy_hip_reads_rem", "sassy_hip_reads_free",
    "sassy_hip_search_hamming_reads", "sassy_hip_hamming_best_pattern_reads", "sassy_hip_hamming_counts_reads",
    "sassy_hip_search_many_reads", "sassy_hip_min_costs_reads", "sassy_hip_best_pattern_reads", "sassy_hip_best_matches_reads",
    "sassy_hip_reads_relayout", "sassy_hip_read_overlaps",
    "sassy_hip_reads_quality", "sassy_hip_merge_pairs",
    "sassy_hip_trim_reads", "sassy_hip_reads_slice",
    "sassy_hip_reads_select", "sassy_hip_demux_reads",
    "sassy_hip_umi_groups_reads", "sassy_hip_dedup_reads",
]

_lib = None


def library_path() -> str:
    return _SO


def lib():
    """The loaded C-ABI library.  Fails loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise SassyHipError(
            f"{_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc, gfx950).  There is no pure-Python / CPU fallback for the search path.")
    L = C.CDLL(_SO)
    vp, u8p, sz = C.c_void_p, C.c_char_p, C.c_size_t
    L.sassy_hip_last_error.restype = C.c_char_p
    L.sassy_hip_version.restype = C.c_char_p
    L.sassy_hip_device_count.restype = C.c_int
    L.sassy_hip_searcher_new.restype = vp
    L.sassy_hip_searcher_new.argtypes = [C.c_char_p, C.c_bool, C.c_float]
    L.sassy_searcher.restype = vp
    L.sassy_searcher.argtypes = [C.c_char_p, C.c_bool, C.c_float]
    L.sassy_searcher_free.restype = None
    L.sassy_searcher_free.argtypes = [vp]
    L.search.restype = sz
    L.search.argtypes = [vp, u8p, sz, u8p, sz, sz, C.POINTER(C.POINTER(CMatch))]
    L.sassy_matches_free.restype = None
    L.sassy_matches_free.argtypes = [C.POINTER(CMatch), sz]
    L.sassy_hip_set_stream.restype = C.c_int
    L.sassy_hip_set_stream.argtypes = [vp, vp]
    L.sassy_hip_get_stats.restype = C.c_int
    L.sassy_hip_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.sassy_hip_enable_counters.restype = C.c_int
    L.sassy_hip_enable_counters.argtypes = [vp, C.c_int]
    L.sassy_hip_set_timing.restype = C.c_int
    L.sassy_hip_set_timing.argtypes = [vp, C.c_int]
    L.sassy_hip_set_prefilter.restype = C.c_int
    L.sassy_hip_set_prefilter.argtypes = [vp, C.c_int]
    L.sassy_hip_set_fused.restype = C.c_int
    L.sassy_hip_set_fused.argtypes = [vp, C.c_int]
    L.sassy_hip_set_option.restype = C.c_int
    L.sassy_hip_set_option.argtypes = [vp, C.c_char_p, C.c_long]
    L.sassy_hip_get_option.restype = C.c_int
    L.sassy_hip_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_long)]
    L.sassy_hip_option_table.restype = C.c_char_p
    L.sassy_hip_option_table.argtypes = []
    L.sassy_hip_set_device.restype = C.c_int
    L.sassy_hip_set_device.argtypes = [vp, C.c_int]
    L.sassy_hip_get_device.restype = C.c_int
    L.sassy_hip_get_device.argtypes = [vp]
    L.sassy_hip_merge_shards.restype = C.c_int
    L.sassy_hip_merge_shards.argtypes = [C.POINTER(vp), C.c_size_t, C.c_int, C.POINTER(vp)]
    L.sassy_hip_multi_new.restype = vp
    L.sassy_hip_multi_new.argtypes = [C.c_char_p, C.c_float, C.POINTER(C.c_int), C.c_size_t]
    L.sassy_hip_multi_shards.restype = C.c_size_t
    L.sassy_hip_multi_shards.argtypes = [vp]
    L.sassy_hip_multi_device.restype = C.c_int
    L.sassy_hip_multi_device.argtypes = [vp, C.c_size_t]
    L.sassy_hip_multi_searcher.restype = vp
    L.sassy_hip_multi_searcher.argtypes = [vp, C.c_size_t]
    L.sassy_hip_multi_set_text.restype = C.c_int
    L.sassy_hip_multi_set_text.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t]
    L.sassy_hip_multi_generate_dna.restype = C.c_int
    L.sassy_hip_multi_generate_dna.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_size_t, C.c_size_t]
    L.sassy_hip_multi_plant.restype = C.c_int
    L.sassy_hip_multi_plant.argtypes = [vp, C.c_uint64, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sassy_hip_multi_search.restype = C.c_int
    L.sassy_hip_multi_search.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(vp)]
    if hasattr(L, "sassy_hip_multi_set_rc"):  # (an older build loaded for an A/B timing lacks the newer entry points)
        L.sassy_hip_multi_set_rc.restype = C.c_int
        L.sassy_hip_multi_set_rc.argtypes = [vp, C.c_int]
        L.sassy_hip_multi_set_replicated.restype = C.c_int
        L.sassy_hip_multi_set_replicated.argtypes = [vp, C.c_int]
        L.sassy_hip_multi_search_encoded.restype = C.c_int
        L.sassy_hip_multi_search_encoded.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(vp)]
        L.sassy_hip_multi_search_many.restype = C.c_int
        L.sassy_hip_multi_search_many.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                                  C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, C.c_uint32,
                                                  C.POINTER(vp)]
    if hasattr(L, "sassy_hip_multi_search_begin"):
        L.sassy_hip_multi_set_pipe_depth.restype = C.c_int
        L.sassy_hip_multi_set_pipe_depth.argtypes = [vp, C.c_int]
        L.sassy_hip_multi_search_begin.restype = C.c_int
        L.sassy_hip_multi_search_begin.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(vp)]
        L.sassy_hip_multi_search_finish.restype = C.c_int
        L.sassy_hip_multi_search_finish.argtypes = [vp, vp, C.POINTER(vp)]
        L.sassy_hip_multi_layout.restype = C.c_long
        L.sassy_hip_multi_layout.argtypes = [C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)]
    if hasattr(L, "sassy_hip_seed_layout"):
        L.sassy_hip_seed_layout.restype = C.c_long
        L.sassy_hip_seed_layout.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_size_t, C.c_size_t, C.c_size_t,
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    if hasattr(L, "sassy_hip_seed_test_rows"):
        L.sassy_hip_seed_test_rows.restype = C.c_long
        L.sassy_hip_seed_test_rows.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.sassy_hip_multi_free.restype = None
    L.sassy_hip_multi_free.argtypes = [vp]
    L.sassy_hip_set_only_best_match.restype = C.c_int
    L.sassy_hip_set_only_best_match.argtypes = [vp, C.c_int]
    L.sassy_hip_set_max_overhang.restype = C.c_int
    L.sassy_hip_set_max_overhang.argtypes = [vp, C.c_long]
    L.sassy_hip_set_max_n_frac.restype = C.c_int
    L.sassy_hip_set_max_n_frac.argtypes = [vp, C.c_float]
    L.sassy_hip_search_many.restype = C.c_int
    L.sassy_hip_search_many.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t,
                                        C.c_uint32, C.POINTER(vp)]
    L.sassy_hip_tsv_header.restype = C.c_char_p
    for fn, extra in ((L.sassy_hip_min_costs, [vp, vp]), (L.sassy_hip_best_pattern, [vp, vp, vp])):
        fn.restype = C.c_int
        fn.argtypes = list(L.sassy_hip_search_many.argtypes[:-1]) + extra
    L.sassy_hip_best_matches.restype = C.c_int
    L.sassy_hip_best_matches.argtypes = list(L.sassy_hip_search_many.argtypes)
    L.sassy_hip_tsv_header.argtypes = []
    L.sassy_hip_format_tsv.restype = C.c_long
    L.sassy_hip_format_tsv.argtypes = [vp, C.POINTER(_HipMatch), C.c_char_p, C.c_char_p, C.c_char_p, vp, C.c_size_t,
                                       C.c_int, C.c_char_p, C.c_size_t]
    L.sassy_hip_search_with_fn.restype = C.c_int
    L.sassy_hip_search_with_fn.argtypes = [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_uint32,
                                           END_FILTER, vp, C.POINTER(vp)]
    L.sassy_hip_search.restype = C.c_int
    L.sassy_hip_search.argtypes = [vp, u8p, sz, vp, sz, sz, C.c_uint32, C.POINTER(vp)]
    L.sassy_hip_search_classes.restype = C.c_int
    L.sassy_hip_search_classes.argtypes = [vp, u8p, sz, vp, sz, sz, C.c_uint32, C.POINTER(vp)]
    L.sassy_hip_search_hamming.restype = C.c_int
    L.sassy_hip_search_hamming.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, vp, sz, sz, C.c_uint32, C.POINTER(vp)]
    L.sassy_hip_search_hamming_many.restype = C.c_int
    L.sassy_hip_search_hamming_many.argtypes = list(L.sassy_hip_search_many.argtypes)
    L.sassy_hip_hamming_best_pattern.restype = C.c_int
    L.sassy_hip_hamming_best_pattern.argtypes = list(L.sassy_hip_search_many.argtypes[:-1]) + [vp, vp, vp, vp]
    L.sassy_hip_hamming_counts.restype = C.c_int
    L.sassy_hip_hamming_counts.argtypes = list(L.sassy_hip_search_hamming.argtypes[:-1]) + [vp]
    L.sassy_hip_hamming_counts_many.restype = C.c_int
    L.sassy_hip_hamming_counts_many.argtypes = list(L.sassy_hip_search_many.argtypes[:-1]) + [vp]
    L.sassy_hip_hamming_amplicons.restype = C.c_int
    L.sassy_hip_hamming_amplicons.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.POINTER(C.c_char_p), C.POINTER(sz), sz, vp, sz, sz,
                                              C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(vp), C.POINTER(sz)]
    L.sassy_hip_amplicons_free.restype = None
    L.sassy_hip_amplicons_free.argtypes = [vp]
    L.sassy_hip_hamming_pairs.restype = C.c_int
    L.sassy_hip_hamming_pairs.argtypes = [vp, vp, sz, vp, sz, sz, sz, C.c_uint32, C.POINTER(vp), C.POINTER(sz)]
    L.sassy_hip_hamming_pairs_free.restype = None
    L.sassy_hip_hamming_pairs_free.argtypes = [vp]
    L.sassy_hip_hamming_nearest.restype = C.c_int
    L.sassy_hip_hamming_nearest.argtypes = [vp, vp, sz, vp, sz, sz, sz, C.c_uint32, vp, vp, vp, vp]
    L.sassy_hip_edit_pairs.restype = C.c_int
    L.sassy_hip_edit_pairs.argtypes = [vp, vp, sz, sz, vp, sz, sz, sz, C.c_uint32, C.POINTER(vp), C.POINTER(sz)]
    L.sassy_hip_edit_pairs_free.restype = None
    L.sassy_hip_edit_pairs_free.argtypes = [vp]
    L.sassy_hip_edit_nearest.restype = C.c_int
    L.sassy_hip_edit_nearest.argtypes = [vp, vp, sz, sz, vp, sz, sz, sz, C.c_uint32, vp, vp, vp, vp]
    L.sassy_hip_hamming_clusters.restype = C.c_int
    L.sassy_hip_hamming_clusters.argtypes = [vp, vp, sz, sz, sz, C.c_uint32, vp, vp, C.POINTER(sz)]
    L.sassy_hip_edit_clusters.restype = C.c_int
    L.sassy_hip_edit_clusters.argtypes = [vp, vp, sz, sz, sz, C.c_uint32, vp, vp, C.POINTER(sz)]
    L.sassy_hip_umi_groups.restype = C.c_int
    L.sassy_hip_umi_groups.argtypes = [vp, vp, sz, sz, sz, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.POINTER(sz), C.POINTER(sz)]
    L.sassy_hip_class_cover.restype = C.c_long
    L.sassy_hip_class_cover.argtypes = [u8p, vp, vp, sz, C.POINTER(C.c_int)]
    L.sassy_hip_search_all_alignments.restype = C.c_int
    L.sassy_hip_search_all_alignments.argtypes = [vp, u8p, sz, vp, sz, sz, C.c_uint32, C.POINTER(vp)]
    L.sassy_hip_search_shard.restype = C.c_int
    L.sassy_hip_search_shard.argtypes = [vp, u8p, sz, vp, C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.c_uint64, sz, C.c_uint32, C.POINTER(vp)]
    L.sassy_hip_search_shard_begin.restype = C.c_int
    L.sassy_hip_search_shard_begin.argtypes = [vp, u8p, sz, vp, C.c_uint64, C.c_uint64, C.c_uint64,
                                               C.c_uint64, sz, C.c_uint32, C.POINTER(vp)]
    L.sassy_hip_set_reference_lanes.restype = C.c_int
    L.sassy_hip_set_reference_lanes.argtypes = [vp, C.c_int]
    L.sassy_hip_set_geometry_tuner.restype = C.c_int
    L.sassy_hip_set_geometry_tuner.argtypes = [vp, C.c_int]
    L.sassy_hip_set_pipe_depth.restype = C.c_int
    L.sassy_hip_set_pipe_depth.argtypes = [vp, C.c_int]
    L.sassy_hip_search_finish.restype = C.c_int
    L.sassy_hip_search_finish.argtypes = [vp, vp, C.POINTER(vp)]
    L.sassy_hip_required_halo.restype = C.c_uint64
    L.sassy_hip_required_halo.argtypes = [sz, sz]
    L.sassy_hip_result_len.restype = sz
    L.sassy_hip_result_len.argtypes = [vp]
    L.sassy_hip_result_matches.restype = C.POINTER(_HipMatch)
    L.sassy_hip_result_matches.argtypes = [vp]
    L.sassy_hip_result_cigars.restype = vp
    L.sassy_hip_result_cigars.argtypes = [vp]
    L.sassy_hip_result_cigars_len.restype = sz
    L.sassy_hip_result_cigars_len.argtypes = [vp]
    L.sassy_hip_pack_rows.restype = C.c_int
    L.sassy_hip_pack_rows.argtypes = [vp, sz, C.c_char_p, sz, vp, sz]
    L.sassy_hip_result_exit_state.restype = C.c_int
    L.sassy_hip_result_exit_state.argtypes = [vp]
    L.sassy_hip_result_conditional_index.restype = C.c_int64
    L.sassy_hip_result_conditional_index.argtypes = [vp]
    L.sassy_hip_result_free.restype = None
    L.sassy_hip_result_free.argtypes = [vp]
    L.sassy_hip_encode_patterns.restype = vp
    L.sassy_hip_encode_patterns.argtypes = [vp, u8p, sz, sz]
    L.sassy_hip_encoded_free.restype = None
    L.sassy_hip_encoded_free.argtypes = [vp]
    L.sassy_hip_search_encoded.restype = C.c_int
    L.sassy_hip_search_encoded.argtypes = [vp, vp, vp, sz, sz, C.c_uint32, C.POINTER(vp)]
    L.sassy_hip_generate_dna.restype = C.c_int
    L.sassy_hip_generate_dna.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    L.sassy_hip_generate_genome_like.restype = C.c_int
    L.sassy_hip_generate_genome_like.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, vp]
    L.sassy_hip_plant.restype = C.c_int
    L.sassy_hip_plant.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u8p, sz, sz,
                                  C.c_uint64, vp, C.POINTER(C.c_uint64)]
    L.sassy_hip_plant_phase.restype = C.c_int
    L.sassy_hip_plant_phase.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u8p, sz, sz,
                                        C.c_uint64, C.c_uint64, vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "sassy_hip_line_spans"):
        L.sassy_hip_line_spans.restype = C.c_int
        L.sassy_hip_line_spans.argtypes = [vp, vp, sz, C.c_uint32, vp, vp, sz, vp]
        L.sassy_hip_result_line_spans.restype = vp
        L.sassy_hip_result_line_spans.argtypes = [vp]
        L.sassy_hip_line_tile.restype = C.c_uint32
        L.sassy_hip_line_tile.argtypes = []
        L.sassy_hip_line_span_times.restype = C.c_int
        L.sassy_hip_line_span_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sassy_hip_fasta_unwrap.restype = C.c_int
    L.sassy_hip_fasta_unwrap.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.POINTER(vp)]
    L.sassy_hip_fasta_n_records.restype = C.c_uint64
    L.sassy_hip_fasta_n_records.argtypes = [vp]
    L.sassy_hip_fasta_records.restype = vp
    L.sassy_hip_fasta_records.argtypes = [vp]
    L.sassy_hip_fasta_text.restype = vp
    L.sassy_hip_fasta_text.argtypes = [vp]
    L.sassy_hip_fasta_text_bytes.restype = C.c_uint64
    L.sassy_hip_fasta_text_bytes.argtypes = [vp]
    L.sassy_hip_fasta_free.restype = None
    L.sassy_hip_fasta_free.argtypes = [vp]
    L.sassy_hip_fastq_parse.restype = C.c_int
    L.sassy_hip_fastq_parse.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.POINTER(vp)]
    for name, res in (("n", C.c_uint64), ("records", vp), ("text", vp), ("text_bytes", C.c_uint64), ("longest", C.c_uint64), ("rem", vp),
                      ("quality", vp), ("free", None)):
        fn = getattr(L, "sassy_hip_reads_" + name)
        fn.restype, fn.argtypes = res, [vp]
    # the _reads calls: a handle where the _many sibling takes texts, text_lens, n_texts
    pats = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, vp, sz, C.c_uint32]
    L.sassy_hip_search_hamming_reads.restype = C.c_int
    L.sassy_hip_search_hamming_reads.argtypes = pats + [C.POINTER(vp)]
    L.sassy_hip_hamming_best_pattern_reads.restype = C.c_int
    L.sassy_hip_hamming_best_pattern_reads.argtypes = pats + [vp, vp, vp, vp]
    L.sassy_hip_hamming_counts_reads.restype = C.c_int
    L.sassy_hip_hamming_counts_reads.argtypes = pats + [vp]
    L.sassy_hip_search_many_reads.restype = C.c_int
    L.sassy_hip_search_many_reads.argtypes = pats + [C.POINTER(vp)]
    L.sassy_hip_min_costs_reads.restype = C.c_int
    L.sassy_hip_min_costs_reads.argtypes = pats + [vp, vp]
    L.sassy_hip_best_pattern_reads.restype = C.c_int
    L.sassy_hip_best_pattern_reads.argtypes = pats + [vp, vp, vp]
    L.sassy_hip_best_matches_reads.restype = C.c_int
    L.sassy_hip_best_matches_reads.argtypes = pats + [C.POINTER(vp)]
    L.sassy_hip_reads_relayout.restype = C.c_int
    L.sassy_hip_reads_relayout.argtypes = [vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint8, vp, vp]
    L.sassy_hip_read_overlaps.restype = C.c_int
    L.sassy_hip_read_overlaps.argtypes = [vp, vp, vp, C.c_uint32, sz, C.c_uint32, C.c_uint32, vp]
    L.sassy_hip_merge_pairs.restype = C.c_int
    L.sassy_hip_merge_pairs.argtypes = [vp, vp, vp, C.c_uint32, sz, C.c_uint32, C.c_uint32, vp, C.POINTER(vp)]
    L.sassy_hip_trim_reads.restype = C.c_int
    L.sassy_hip_trim_reads.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_uint32, sz, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       vp, C.POINTER(vp)]
    L.sassy_hip_reads_slice.restype = C.c_int
    L.sassy_hip_reads_slice.argtypes = [vp, vp, vp, vp, C.POINTER(vp)]
    L.sassy_hip_reads_select.restype = C.c_int
    L.sassy_hip_reads_select.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, C.POINTER(vp)]
    L.sassy_hip_demux_reads.restype = C.c_int
    L.sassy_hip_demux_reads.argtypes = [vp, vp, C.POINTER(C.c_char_p), sz, sz, C.c_uint32, sz, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(vp)]
    L.sassy_hip_umi_groups_reads.restype = C.c_int
    L.sassy_hip_umi_groups_reads.argtypes = [vp, vp, C.c_uint32, sz, sz, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.POINTER(sz), C.POINTER(sz)]
    L.sassy_hip_dedup_reads.restype = C.c_int
    L.sassy_hip_dedup_reads.argtypes = [vp, vp, C.c_uint32, sz, sz, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(vp)]
    L.sassy_hip_malloc.restype = vp
    L.sassy_hip_malloc.argtypes = [sz]
    L.sassy_hip_free.restype = None
    L.sassy_hip_free.argtypes = [vp]
    L.sassy_hip_memcpy_h2d.restype = C.c_int
    L.sassy_hip_memcpy_h2d.argtypes = [vp, vp, sz]
    L.sassy_hip_memcpy_d2h.restype = C.c_int
    L.sassy_hip_memcpy_d2h.argtypes = [vp, vp, sz]
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise SassyHipError(f"libsassy_hip error {rc}: {lib().sassy_hip_last_error().decode()}")


def device_count() -> int:
    return lib().sassy_hip_device_count()


@dataclass(frozen=True)
class Match:
    """Reference Match (src/search.rs:35-62) with the Python getters' conventions
    (src/python.rs:157-203): strand is '+' or '-', cigar is the SAM string."""
    pattern_idx: int
    text_start: int
    text_end: int
    pattern_start: int
    pattern_end: int
    cost: int
    strand: str
    cigar: str
    text_idx: int = 0

    def sort_key(self):
        return (self.pattern_idx, self.text_start, self.text_end, self.cost, self.strand, self.cigar)


def match_dtype():
    """numpy view of include/sassy_hip.h: sassy_hip_Match (64 bytes)."""
    import numpy as np
    return np.dtype([("pattern_idx", "<u8"), ("text_idx", "<u8"), ("text_start", "<u8"),
                     ("text_end", "<u8"), ("pattern_start", "<u8"), ("pattern_end", "<u8"),
                     ("cost", "<i4"), ("strand", "u1"), ("pad_", "u1", (3,)),
                     ("cigar_off", "<u4"), ("cigar_len", "<u4")])


def line_span_dtype():
    """numpy view of include/sassy_hip.h: sassy_hip_LineSpan (32 bytes)."""
    import numpy as np
    return np.dtype([("line_no", "<u8"), ("last_line_no", "<u8"), ("line_start", "<u8"), ("line_end", "<u8")])


def amplicon_dtype():
    """numpy view of include/sassy_hip.h: sassy_hip_Amplicon (24 bytes)."""
    import numpy as np
    return np.dtype([("start", "<u8"), ("end", "<u8"), ("pair_idx", "<u4"), ("strand", "u1"), ("fwd_cost", "u1"), ("rev_cost", "u1"),
                     ("pad_", "u1")])


def hamming_pair_dtype():
    """numpy view of include/sassy_hip.h: sassy_hip_HammingPair (12 bytes)."""
    import numpy as np
    return np.dtype([("a_idx", "<u4"), ("b_idx", "<u4"), ("cost", "u1"), ("strand", "u1"), ("pad_", "u1", (2,))])


def pairs_sequences(seqs, who: str = "hamming_pairs"):
    """One list of equal-length sequences for `Searcher.hamming_pairs` / `hamming_nearest` as the (n, m) uint8 array the C
    call reads back to back: a C-contiguous uint8 array of shape (n, m) is used as it is (no copy per entry), a list of bytes
    is joined -- unequal lengths raise SassyHipError naming the first offender.  ClassPattern entries are refused."""
    import numpy as np
    if isinstance(seqs, np.ndarray):
        if seqs.dtype != np.uint8 or seqs.ndim != 2 or not seqs.flags["C_CONTIGUOUS"]:
            raise SassyHipError(f"{who} takes a C-contiguous uint8 array of shape (n, m), or a list of equal-length bytes")
        return seqs
    if isinstance(seqs, ClassPattern) or isinstance(seqs, (bytes, bytearray, memoryview, str)):
        raise SassyHipError(f"{who} takes a list of equal-length byte sequences: a ClassPattern is not supported"
                            if isinstance(seqs, ClassPattern) else f"{who} takes a list of equal-length byte sequences, not one sequence")
    seqs = list(seqs)
    if any(isinstance(p, ClassPattern) for p in seqs):
        raise SassyHipError(f"{who} takes byte sequences only: a ClassPattern is not supported")
    seqs = [bytes(p) for p in seqs]
    m = len(seqs[0]) if seqs else 0
    for i, p in enumerate(seqs):
        if len(p) != m:
            raise SassyHipError(f"{who} takes sequences of one length: sequence {i} has {len(p)} bytes, sequence 0 has {m}")
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), m)


def fasta_record_dtype():
    """numpy view of include/sassy_hip.h: sassy_hip_FastaRecord (32 bytes)."""
    import numpy as np
    return np.dtype([("id_start", "<u8"), ("id_len", "<u8"), ("seq_start", "<u8"), ("seq_len", "<u8")])


def read_record_dtype():
    """numpy view of include/sassy_hip.h: sassy_hip_ReadRecord (48 bytes)."""
    import numpy as np
    return np.dtype([("id_start", "<u8"), ("id_len", "<u8"), ("seq_start", "<u8"), ("seq_len", "<u8"), ("qual_start", "<u8"),
                     ("qual_len", "<u8")])


def read_overlap_dtype():
    """numpy view of include/sassy_hip.h: sassy_hip_ReadOverlap (16 bytes)."""
    import numpy as np
    return np.dtype([("offset", "<i4"), ("overlap", "<u4"), ("mismatches", "<u4"), ("n_accepted", "<u4")])


def read_trim_dtype():
    """numpy view of include/sassy_hip.h: sassy_hip_ReadTrim (16 bytes)."""
    import numpy as np
    return np.dtype([("length", "<u4"), ("quality_len", "<u4"), ("adapter_pos", "<u4"), ("adapter", "<i2"), ("overlap", "u1"), ("mismatches", "u1")])


def read_demux_dtype():
    """numpy view of include/sassy_hip.h: sassy_hip_ReadDemux (16 bytes)."""
    import numpy as np
    return np.dtype([("sample", "<i4"), ("best", "<u4"), ("cost", "u1"), ("second", "u1"), ("n_best", "<u2"), ("index", "<u4")])


OVERLAP_MAX_LEN = 512  # SASSY_HIP_OVERLAP_MAX_LEN
TRIM_MAX_ADAPTERS = 64  # SASSY_HIP_TRIM_MAX_ADAPTERS
DEMUX_MAX_BARCODES = 4096  # SASSY_HIP_DEMUX_MAX_BARCODES
DEMUX_END3 = 1  # SASSY_HIP_DEMUX_END3
DEDUP_END3 = 1  # SASSY_HIP_DEDUP_END3
DEMUX_KEEP_BARCODE = 2  # SASSY_HIP_DEMUX_KEEP_BARCODE


def overlap_trims(rec, la: int, lb: int):
    """(insert, keep1, keep2) of one record of `Searcher.read_overlaps` for reads of la and lb bytes: the fragment length and
    how many bytes of each read belong to it.  d >= 0: insert = max(la, d + lb), both reads are kept whole; d < 0
    (read-through: the tails are adapter): insert = ov, keep1 = min(la, d + lb), keep2 = lb + d; no overlap (n_accepted == 0):
    insert = 0 and both reads whole.  Pure arithmetic on the host."""
    d, ov, n = int(rec["offset"]), int(rec["overlap"]), int(rec["n_accepted"])
    la, lb = int(la), int(lb)
    if n == 0:
        return 0, la, lb
    if d >= 0:
        return max(la, d + lb), la, lb
    return ov, min(la, d + lb), lb + d


def fastq_from_sequences(seqs, quals=None) -> bytes:
    """Minimal four-line FASTQ of a list of byte sequences, an empty id and an empty quality each: b"@\\n" + seq + b"\\n+\\n\\n".
    A sequence that holds a line end would change the record structure and is refused.  `quals`: a list of as many quality
    strings, each as long as its sequence and free of line ends, which take the place of the empty quality lines."""
    if quals is not None and len(quals) != len(seqs):
        raise SassyHipError(f"from_sequences: {len(seqs)} sequences and {len(quals)} qualities")
    out = []
    for i, s in enumerate(seqs):
        if isinstance(s, str):
            s = s.encode()
        s = bytes(s)
        if b"\n" in s or b"\r" in s:
            raise SassyHipError(f"from_sequences: sequence {i} holds a line end (\\n or \\r)")
        q = b""
        if quals is not None:
            q = quals[i].encode() if isinstance(quals[i], str) else bytes(quals[i])
            if b"\n" in q or b"\r" in q:
                raise SassyHipError(f"from_sequences: quality {i} holds a line end (\\n or \\r)")
            if len(q) != len(s):
                raise SassyHipError(f"from_sequences: quality {i} has {len(q)} bytes, its sequence {len(s)}")
        out.append(b"@\n" + s + b"\n+\n" + q + b"\n")
    return b"".join(out)


def reads_to_fastq(reads, ids) -> bytes:
    """FASTQ of a DeviceReads with kept qualities (a merged batch of `Searcher.merge_pairs`, say): record r is written under
    ids[r] (str or bytes, without the '@'), empty records are skipped.  Two downloads -- the text and the quality buffer --
    sliced with numpy on the host."""
    import numpy as np
    if len(ids) != len(reads):
        raise SassyHipError(f"reads_to_fastq: {len(reads)} reads and {len(ids)} ids")
    text = np.frombuffer(reads.download_text(), dtype=np.uint8)
    qual = np.frombuffer(reads.download_quality_text(), dtype=np.uint8)
    keep = np.flatnonzero(reads.seq_lens)
    if not keep.size:
        return b""
    lens = reads.seq_lens[keep].astype(np.int64)
    starts = reads.seq_starts[keep].astype(np.int64)
    heads = [b"@" + (i.encode() if isinstance(i, str) else bytes(i)) + b"\n" for i in (ids[r] for r in keep.tolist())]
    head_lens = np.array([len(h) for h in heads], dtype=np.int64)
    rec_lens = head_lens + 2 * lens + 4  # '@id\n' seq '\n+\n' qual '\n'
    at = np.concatenate([[0], np.cumsum(rec_lens)[:-1]])
    out = np.empty(int(rec_lens.sum()), dtype=np.uint8)
    # the bytes of every sequence (and quality) as one gather: source index = start + the position within its read
    within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    src = np.repeat(starts, lens) + within
    seq_at = at + head_lens
    out[np.repeat(seq_at, lens) + within] = text[src]
    out[np.repeat(seq_at + lens + 3, lens) + within] = qual[src]
    out[np.repeat(at, head_lens) + (np.arange(int(head_lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(head_lens) - head_lens, head_lens))] = \
        np.frombuffer(b"".join(heads), dtype=np.uint8)
    mid = seq_at + lens  # '\n+\n' between the sequence and the quality, '\n' behind the quality
    out[mid], out[mid + 1], out[mid + 2], out[mid + 3 + lens] = 10, 43, 10, 10
    return out.tobytes()


def line_tile() -> int:
    """Text bytes per tile of the device's line index (sassy_hip_line_tile)."""
    return lib().sassy_hip_line_tile()


def _bytes_at(addr, size: int) -> bytes:
    """`size` bytes at a C address (ctypes.string_at takes an int-sized length: results above 2 GiB need the array form)."""
    if not size:
        return b""
    if size < (1 << 31):
        return C.string_at(addr, size)
    return bytes((C.c_char * size).from_address(addr if isinstance(addr, int) else C.cast(addr, C.c_void_p).value))


class Result:
    """Matches of one call plus the shard bookkeeping (see include/sassy_hip.h).

    ``array`` is the C match array copied once into a numpy structured array (match_dtype) and
    ``pool`` the cigar string pool; ``matches`` materialises reference-style Match objects on
    first use (a Python object per match is far slower than the search itself)."""

    def __init__(self, handle, flags: int = 0):
        # The C call has left the finished records on the host (sassy_hip_Result); they are copied into
        # Python objects only when somebody looks at them (`array`, `pool`, `matches`).
        L = lib()
        self._h = handle
        self._n = L.sassy_hip_result_len(handle)
        self.exit_state = L.sassy_hip_result_exit_state(handle)
        self.conditional_index = L.sassy_hip_result_conditional_index(handle)
        self._array = None
        self._pool = None
        self._matches = None
        self._line_spans = None
        self._flags = flags  # of the call: LINE_SPANS decides whether `line_spans` is an array (empty, too) or None

    def _materialise(self):
        if self._array is not None:
            return
        import numpy as np
        L = lib()
        h, self._h = self._h, None
        try:
            n = self._n
            ptr = L.sassy_hip_result_matches(h)
            raw = _bytes_at(ptr, n * 64)
            self._array = np.frombuffer(raw, dtype=match_dtype())
            plen = L.sassy_hip_result_cigars_len(h)
            pool = L.sassy_hip_result_cigars(h)
            self._pool = _bytes_at(pool, plen)
            if self._flags & LINE_SPANS:  # (an empty result has no array to point at: n == 0 reads nothing)
                spans = L.sassy_hip_result_line_spans(h)
                self._line_spans = np.frombuffer(_bytes_at(spans, n * 32), dtype=line_span_dtype())
        finally:
            L.sassy_hip_result_free(h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().sassy_hip_result_free(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    @property
    def array(self):
        """The C match array copied once into a numpy structured array (match_dtype)."""
        self._materialise()
        return self._array

    @property
    def line_spans(self):
        """The matches' lines as a numpy structured array (line_span_dtype), parallel to `array` -- None unless the search
        ran with LINE_SPANS (Searcher.search_lines)."""
        self._materialise()
        return self._line_spans

    @property
    def pool(self) -> bytes:
        """The cigar string pool."""
        self._materialise()
        return self._pool

    def __len__(self):
        return self._n

    @property
    def matches(self) -> List["Match"]:
        """The records as reference-style Match objects -- always a real list, whatever the size of the result (a Python
        object per match costs 1.4 us: for results of 10^5 records and more use `.lazy_matches` or the numpy `.array`)."""
        if self._matches is None:
            self._matches = matches_from_array(self.array, self.pool)
        return self._matches

    @property
    def lazy_matches(self) -> "MatchList":
        """A read-only sequence over the numpy array and the cigar pool: Match objects are made when they are looked at."""
        return MatchList(self.array, self.pool)


def _bytes_payload_offset():
    """Where the payload of a bytes object sits behind id(obj) -- CPython's object layout, checked once at import against a
    known string; None (search_many then takes every text through _ptr_len) on any other interpreter or layout, or where
    a pointer does not fit the uint64 / size_t arrays the fast path builds."""
    import sys
    if sys.implementation.name != "cpython" or C.sizeof(C.c_void_p) != 8 or C.sizeof(C.c_size_t) != 8:
        return None
    off = bytes.__basicsize__ - 1
    probe = b"sassy-layout-probe"
    try:
        return off if C.string_at(id(probe) + off, len(probe)) == probe else None
    except Exception:
        return None


_BYTES_PAYLOAD_OFFSET = _bytes_payload_offset()


class MatchList(_SequenceABC):
    """A read-only sequence of Match objects over a Result's numpy array and cigar pool: len(), indexing, slicing and
    iteration behave like the list they replace, the objects are made when they are looked at.  `.array` / `.pool`:
    the columns themselves (match_dtype)."""

    __slots__ = ("array", "pool")

    def __init__(self, array, pool: bytes):
        self.array = array
        self.pool = pool

    def __len__(self):
        return len(self.array)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return matches_from_array(self.array[i], self.pool)
        return matches_from_array(self.array[i:i + 1] if i >= 0 else self.array[len(self.array) + i:len(self.array) + i + 1],
                                  self.pool)[0]

    def __iter__(self):
        for a in range(0, len(self.array), 4096):
            yield from matches_from_array(self.array[a:a + 4096], self.pool)

    def __eq__(self, other):
        if isinstance(other, (list, tuple, MatchList)):
            return len(other) == len(self) and all(x == y for x, y in zip(self, other))
        return NotImplemented

    def __repr__(self):
        return f"MatchList({len(self)} matches)"


def matches_from_array(array, pool: bytes) -> List["Match"]:
    out = []
    for r in array.tolist():
        (pidx, tidx, ts, te, ps, pe, cost, strand, _pad, coff, clen) = r
        out.append(Match(pidx, ts, te, ps, pe, cost, "-" if strand else "+",
                         pool[coff:coff + clen].decode() if clen else "", tidx))
    return out


def _ptr_len(text):
    """(address, length, keepalive, on_device) for bytes / numpy uint8 / torch uint8 tensors."""
    if isinstance(text, (bytes, bytearray)):
        b = bytes(text)
        return C.cast(C.c_char_p(b), C.c_void_p).value or 0, len(b), b, False
    if hasattr(text, "data_ptr"):  # torch tensor
        if text.dtype.itemsize != 1 or not text.is_contiguous():
            raise SassyHipError("text tensor must be contiguous uint8")
        return text.data_ptr(), text.numel(), text, text.is_cuda
    if hasattr(text, "ctypes"):  # numpy
        import numpy as np
        a = np.ascontiguousarray(text, dtype=np.uint8)
        return a.ctypes.data, a.size, a, False
    raise TypeError("text must be bytes, a numpy uint8 array or a torch uint8 tensor")


class TextBatch:
    """Many host texts as ONE buffer and two arrays: text i = buffer[starts[i] : starts[i] + lens[i]].  What a FASTA /
    FASTQ reader holds anyway; `search_many` takes it without touching a Python object per text (a list of 330 000
    `bytes` costs 25 ms to marshal -- more than the search).  `TextBatch.from_list(texts)` packs a list once, for
    several calls."""

    def __init__(self, buffer, starts, lens):
        import numpy as np
        self.buffer = np.ascontiguousarray(np.frombuffer(buffer, dtype=np.uint8) if isinstance(buffer, (bytes, bytearray, memoryview))
                                           else buffer, dtype=np.uint8)
        self.starts = np.ascontiguousarray(starts, dtype=np.uint64)
        self.lens = np.ascontiguousarray(lens, dtype=np.uint64)
        if self.starts.shape != self.lens.shape or self.starts.ndim != 1:
            raise SassyHipError("TextBatch: starts and lens must be one-dimensional and of one length")
        if len(self.starts) and int((self.starts + self.lens).max()) > self.buffer.size:
            raise SassyHipError("TextBatch: a text ends behind the buffer")
        self._addr = self.starts + np.uint64(self.buffer.ctypes.data)  # (the buffer is kept alive by self)

    @classmethod
    def from_list(cls, texts: Sequence[bytes]) -> "TextBatch":
        import numpy as np
        lens = np.fromiter(map(len, texts), dtype=np.uint64, count=len(texts))
        starts = np.zeros(len(texts), dtype=np.uint64)
        if len(texts) > 1:
            np.cumsum(lens[:-1], out=starts[1:])
        return cls(b"".join(texts), starts, lens)

    def __len__(self):
        return len(self.starts)


class EncodedPatterns:
    """Reference EncodedPatterns (src/pattern_tiling/general.rs:132-150), opaque."""

    def __init__(self, handle, n, plen):
        self._h, self.n_patterns, self.pattern_len = handle, n, plen

    def __del__(self):
        if getattr(self, "_h", None):
            lib().sassy_hip_encoded_free(self._h)
            self._h = None


class ClassPattern:
    """A character-class pattern: m positions, each a set of byte values.  `sets` holds 32 bytes per position -- byte value
    c belongs to position j iff bit c & 7 of sets[32 j + (c >> 3)] is set (the layout sassy_hip_search_classes takes)."""

    def __init__(self, sets: bytes):
        sets = bytes(sets)
        if len(sets) % 32:
            raise SassyHipError("ClassPattern: 32 bytes per position")
        self.sets = sets
        self.m = len(sets) // 32

    @classmethod
    def from_sets(cls, sets) -> "ClassPattern":
        """One iterable of byte values (ints, or a bytes object) per position."""
        out = bytearray()
        for members in sets:
            out += _set_bytes(members)
        return cls(bytes(out))

    def members(self, j: int) -> List[int]:
        return [c for c in range(256) if (self.sets[32 * j + (c >> 3)] >> (c & 7)) & 1]

    def __len__(self):
        return self.m

    def __eq__(self, other):
        return isinstance(other, ClassPattern) and self.sets == other.sets

    def __repr__(self):
        return "ClassPattern(m=%d)" % self.m


def _set_bytes(members) -> bytearray:
    b = bytearray(32)
    for c in members:
        c = int(c)
        if not 0 <= c < 256:
            raise SassyHipError("a class holds byte values 0 .. 255, got %d" % c)
        b[c >> 3] |= 1 << (c & 7)
    return b


_CLASS_ESCAPES = {
    ord("d"): frozenset(range(ord("0"), ord("9") + 1)),
    ord("w"): frozenset(list(range(ord("0"), ord("9") + 1)) + list(range(ord("A"), ord("Z") + 1)) +
                        list(range(ord("a"), ord("z") + 1)) + [ord("_")]),
    ord("s"): frozenset(b" \t\n\r\f\v"),
}
_ALL_BYTES = frozenset(range(256))


def parse_classes(expr: bytes) -> ClassPattern:
    """The class pattern of an expression, one element per position: a literal byte; `.` (every byte but '\\n');
    `[...]` with ranges and a leading `^` (the complement over all 256 byte values; a `]` right behind `[` or `[^` is a
    member); the escapes \\d \\D \\w \\W \\s \\S (also inside brackets), \\n \\t \\xHH and an escaped . [ ] \\ ^ -.  No
    quantifiers, alternation or anchors.  Raises SassyHipError with the offset of what it cannot read."""
    if isinstance(expr, str):
        expr = expr.encode()
    expr = bytes(expr)
    n = len(expr)
    if n == 0:
        raise SassyHipError("empty class expression (offset 0)")

    def escape(i):
        """The escape whose backslash sits at i: (set of members, next offset)."""
        if i + 1 >= n:
            raise SassyHipError("trailing backslash at offset %d" % i)
        c = expr[i + 1]
        if c in b"dDwWsS":
            base = _CLASS_ESCAPES[c | 0x20]
            return (base if c & 0x20 else _ALL_BYTES - base), i + 2
        if c == ord("n"):
            return frozenset([10]), i + 2
        if c == ord("t"):
            return frozenset([9]), i + 2
        if c == ord("x"):
            hx = expr[i + 2:i + 4]
            try:
                if len(hx) != 2:
                    raise ValueError
                return frozenset([int(hx.decode("ascii"), 16)]), i + 4
            except ValueError:
                raise SassyHipError("\\x needs two hex digits at offset %d" % i) from None
        if c in b".[]\\^-":
            return frozenset([c]), i + 2
        raise SassyHipError("unknown escape \\%s at offset %d" % (chr(c), i))

    sets = []
    i = 0
    while i < n:
        c = expr[i]
        if c == ord("\\"):
            members, i = escape(i)
        elif c == ord("."):
            members, i = _ALL_BYTES - {10}, i + 1
        elif c == ord("["):
            start = i
            i += 1
            negate = i < n and expr[i] == ord("^")
            if negate:
                i += 1
            members = set()
            first = True
            while True:
                if i >= n:
                    raise SassyHipError("unterminated class opened at offset %d" % start)
                c = expr[i]
                if c == ord("]") and not first:
                    i += 1
                    break
                first = False
                if c == ord("\\"):
                    lo_set, nxt = escape(i)
                    if len(lo_set) != 1:  # \d and its kin: no range ends
                        members |= lo_set
                        i = nxt
                        continue
                    lo = next(iter(lo_set))
                else:
                    lo, nxt = c, i + 1
                # a range lo-hi ('-' right in front of the closing bracket is a member)
                if nxt + 1 < n and expr[nxt] == ord("-") and expr[nxt + 1] != ord("]"):
                    at = nxt + 1
                    if expr[at] == ord("\\"):
                        hi_set, nxt2 = escape(at)
                        if len(hi_set) != 1:
                            raise SassyHipError("a range cannot end in a class escape at offset %d" % at)
                        hi = next(iter(hi_set))
                    else:
                        hi, nxt2 = expr[at], at + 1
                    if hi < lo:
                        raise SassyHipError("reversed range at offset %d" % i)
                    members |= set(range(lo, hi + 1))
                    i = nxt2
                else:
                    members.add(lo)
                    i = nxt
            if negate:
                members = _ALL_BYTES - members
        else:
            members, i = frozenset([c]), i + 1
        sets.append(members)
    return ClassPattern.from_sets(sets)


def class_cover(members):
    """The cube cover the library gives one set (sassy_hip_class_cover; host only): (cubes, complemented) with cubes a
    list of (value, care) -- byte c is in a cube iff (c ^ value) & care == 0; complemented: they cover the complement."""
    st = bytes(_set_bytes(members))
    value = (C.c_uint8 * 128)()
    care = (C.c_uint8 * 128)()
    inv = C.c_int(0)
    n = lib().sassy_hip_class_cover(st, value, care, 128, C.byref(inv))
    if n < 0:
        raise SassyHipError(lib().sassy_hip_last_error().decode())
    return [(value[i], care[i]) for i in range(n)], bool(inv.value)


def _byte_pattern(pattern) -> bytes:
    if isinstance(pattern, ClassPattern):
        raise SassyHipError("this call takes byte patterns only: a class pattern runs through Searcher.search_classes")
    return bytes(pattern)


class _ReadBatchCalls:
    """The Searcher calls that turn one resident read batch into another (self._h: the searcher's handle).  They live in a base
    class of Searcher: each makes a new DeviceReads out of a DeviceReads and keeps nothing of the search family's state."""

    def trim_reads(self, reads, adapters, min_overlap: int = 3, k: int = OVERLAP_MAX_LEN, max_permille: int = 100, quality_cutoff: int = 0,
                   min_length: int = 0, with_records: bool = False):
        """The 3' adapter and the low-quality tail cut off every read on the device (sassy_hip_trim_reads).  Quality first
        (`quality_cutoff` > 0: the BWA / cutadapt rule on Phred+33, which leaves lq bytes), then the adapters on what is left:
        position c places an adapter's first byte under a[c], it overlaps in ov = min(m, lq - c) rows, and c is accepted with
        at least `min_overlap` rows, at most `k` mismatches and at most `max_permille` per thousand of them.  The leftmost
        accepted position wins, then the lower density, the longer overlap, the earlier adapter; the read is cut there, and
        a read left shorter than `min_length` becomes empty.  Returns a new DeviceReads, ONE RECORD PER READ, with qualities
        iff the input has them, which every call that takes a DeviceReads takes; with `with_records` also a numpy array of
        `read_trim_dtype()`.  `reads`: a DeviceReads, or a list of sequences or of (sequence, quality) tuples.  `adapters`:
        up to 64 byte strings of 1 .. 64 bytes, 5'->3' as they follow the insert; none: quality and length trimming only.
        dna (A, C, G, T only) or iupac.  The definition is tests/helpers/trim_reads_ref.py."""
        import numpy as np
        adapters = [a.encode() if isinstance(a, str) else _byte_pattern(a) for a in adapters]
        made = None
        if not isinstance(reads, DeviceReads):
            reads = list(reads)
            paired = bool(reads) and isinstance(reads[0], tuple)
            made = reads = DeviceReads.from_sequences([x[0] for x in reads], [x[1] for x in reads]) if paired else DeviceReads.from_sequences(reads)
        try:
            numbers = (min_overlap, max_permille, quality_cutoff, min_length)
            if any(not 0 <= int(v) < (1 << 32) for v in numbers) or int(k) < 0:
                raise SassyHipError("trim_reads: min_overlap, max_permille, quality_cutoff and min_length must fit 32 bits, and none of them nor k may be negative")
            ptrs = (C.c_char_p * max(len(adapters), 1))(*adapters)
            lens = (C.c_size_t * max(len(adapters), 1))(*[len(a) for a in adapters])
            records = np.zeros(len(reads), dtype=read_trim_dtype()) if with_records else None
            out = C.c_void_p()
            _check(lib().sassy_hip_trim_reads(self._h, reads._handle(), ptrs, lens, len(adapters), int(min_overlap), int(k), int(max_permille),
                                              int(quality_cutoff), int(min_length), 0,
                                              records.ctypes.data if with_records and len(records) else None, C.byref(out)))
            trimmed = DeviceReads._adopt(out)
            return (trimmed, records) if with_records else trimmed
        finally:
            if made is not None:
                made.free()


class Searcher(_ReadBatchCalls):
    """Mirror of sassy.Searcher (src/python.rs:26-64) / Searcher::<P>::new (src/search.rs:486-503).

    Note the reference's Python default rc=True; ``new_fwd``-style searchers pass rc=False."""

    def __init__(self, alphabet: str, rc: bool = True, alpha: Optional[float] = None):
        L = lib()
        a = float("nan") if alpha is None else float(alpha)
        self._h = L.sassy_hip_searcher_new(alphabet.encode(), bool(rc), a)
        if not self._h:
            raise SassyHipError(L.sassy_hip_last_error().decode())
        self.alphabet, self.rc = alphabet.lower(), bool(rc)

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().sassy_searcher_free(self._h)
            except Exception:  # interpreter shutdown: the module globals may be gone already
                pass
            self._h = None

    # --- reference API ---
    def search(self, pattern: bytes, text, k: int) -> List[Match]:
        return self._search(pattern, text, k, 0).matches

    def search_all(self, pattern: bytes, text, k: int) -> List[Match]:
        return self._search(pattern, text, k, ALL_MINIMA).matches

    def search_without_trace(self, pattern: bytes, text, k: int) -> List[Match]:
        return self._search(pattern, text, k, WITHOUT_TRACE).matches

    def line_spans(self, text, first, last):
        """Where the spans [first[i], last[i]] of text positions lie, line-wise ('\\n' is the only separator): a numpy
        structured array (line_span_dtype) -- line_no / last_line_no (1-based) of the two ends, line_start of the first,
        line_end of the last; text[line_start:line_end] is the line without its newline.  first <= last <= len(text); a
        match is the span (text_start, max(text_start, text_end - 1)).  Resolved on the device (csrc/line_index.hip) in one
        pass over the text plus one wavefront per span.  `text` as for `search`: bytes, numpy, or a device tensor."""
        import numpy as np
        addr, n, keep, on_dev = _ptr_len(text)
        first = np.ascontiguousarray(first, dtype=np.uint64)
        last = np.ascontiguousarray(last, dtype=np.uint64)
        if first.shape != last.shape or first.ndim != 1:
            raise SassyHipError("line_spans: first and last must be one-dimensional and of one length")
        out = np.empty(len(first), dtype=line_span_dtype())
        _check(lib().sassy_hip_line_spans(self._h, addr, n, TEXT_ON_DEVICE if on_dev else 0, first.ctypes.data, last.ctypes.data,
                                          len(first), out.ctypes.data))
        return out

    def search_lines(self, pattern: bytes, text, k: int, all_minima: bool = False):
        """`search` (or `search_all`) plus the line every match lies in: (matches, spans) -- spans as `line_spans` gives
        them, parallel to the matches, resolved by the same call while the text is resident (a host text is uploaded
        once)."""
        r = self._search(pattern, text, k, LINE_SPANS | (ALL_MINIMA if all_minima else 0))
        return r.matches, r.line_spans

    def search_classes(self, pattern, text, k: int, all_minima: bool = False, without_trace: bool = False, lines: bool = False):
        """`search` / `search_all` / `search_without_trace` for a character-class pattern (sassy_hip_search_classes): a
        ClassPattern, or an expression for `parse_classes`.  Row j matches text byte c iff c is in set j; '=' in the cigar
        is a member, 'X' a non-member.  The searcher's alphabet is "ascii" or "ascii_ci" (every set is then closed under
        the case twin), rc=False, no alpha.  lines=True: (matches, spans) as `search_lines`.  `text` as for `search`."""
        if not isinstance(pattern, ClassPattern):
            pattern = parse_classes(pattern)
        flags = (ALL_MINIMA if all_minima else 0) | (WITHOUT_TRACE if without_trace else 0) | (LINE_SPANS if lines else 0)
        addr, n, keep, on_dev = _ptr_len(text)
        if on_dev:
            flags |= TEXT_ON_DEVICE
            if getattr(self, "_text_unchanged", False):
                flags |= TEXT_UNCHANGED
        out = C.c_void_p()
        _check(lib().sassy_hip_search_classes(self._h, pattern.sets, pattern.m, addr, n, k, flags, C.byref(out)))
        r = Result(out, flags)
        return (r.matches, r.line_spans) if lines else r.matches

    def search_hamming(self, patterns, text, k: int, without_trace: bool = False, as_result: bool = False):
        """Every start with at most k MISMATCHES (substitutions only) of every pattern in one text (sassy_hip_search_hamming):
        one Match per hit -- text_start = s, text_end = s + m, cost = the number of mismatching rows under the searcher's
        profile relation, a cigar of '=' / 'X' runs --, every hit (no local-minimum rule), ordered by (pattern_idx, '+'
        before '-', text_start).  An rc searcher also reports reverse_complement(pattern) on the forward text as strand
        '-', cigar in pattern direction.  `patterns`: bytes, or a sequence of bytes of any lengths -- they share one pass
        over the text; `text` as for `search`.  without_trace: the same records without cigar.  as_result: the Result."""
        if isinstance(patterns, ClassPattern) or (not isinstance(patterns, (bytes, bytearray, memoryview)) and
                                                  any(isinstance(p, ClassPattern) for p in patterns)):
            raise SassyHipError("search_hamming takes byte patterns only: a ClassPattern is not supported")
        if isinstance(patterns, (bytes, bytearray, memoryview)):
            patterns = [patterns]
        patterns = [bytes(p) for p in patterns]
        pp = (C.c_char_p * len(patterns))(*patterns)
        pl = (C.c_size_t * len(patterns))(*[len(p) for p in patterns])
        flags = WITHOUT_TRACE if without_trace else 0
        addr, n, keep, on_dev = _ptr_len(text)
        if on_dev:
            flags |= TEXT_ON_DEVICE
            if getattr(self, "_text_unchanged", False):
                flags |= TEXT_UNCHANGED
        out = C.c_void_p()
        _check(lib().sassy_hip_search_hamming(self._h, pp, pl, len(patterns), addr, n, k, flags, C.byref(out)))
        r = Result(out)
        return r if as_result else r.matches

    @staticmethod
    def _hamming_patterns(patterns, who: str):
        if isinstance(patterns, ClassPattern) or (not isinstance(patterns, (bytes, bytearray, memoryview)) and
                                                  any(isinstance(p, ClassPattern) for p in patterns)):
            raise SassyHipError(f"{who} takes byte patterns only: a ClassPattern is not supported")
        if isinstance(patterns, (bytes, bytearray, memoryview)):
            patterns = [patterns]
        return [bytes(p) for p in patterns]

    @staticmethod
    def _pattern_arrays(patterns):
        return (C.c_char_p * max(1, len(patterns)))(*patterns), (C.c_size_t * max(1, len(patterns)))(*[len(p) for p in patterns])

    def search_hamming_many(self, patterns, texts: Sequence, k: int, without_trace: bool = False, as_result: bool = False):
        """search_hamming over a batch of texts (reads) in one call (sassy_hip_search_hamming_many): the records of
        search_hamming(patterns, texts[t], k) for every t, each with text_idx = t and coordinates relative to its text,
        ordered by (pattern_idx, '+' before '-', text_idx, text_start).  `texts`: a list of host texts or a TextBatch, as
        search_many (host texts only), or a DeviceReads -- a read batch parsed on the device, scanned where it lies
        (sassy_hip_search_hamming_reads; hamming_best_pattern and hamming_counts_many take one likewise).  without_trace: the same records without cigar.  as_result: the Result."""
        patterns = self._hamming_patterns(patterns, "search_hamming_many")
        if isinstance(texts, DeviceReads):  # a resident read batch: sassy_hip_search_hamming_reads
            pp, pl = self._pattern_arrays(patterns)
            out = C.c_void_p()
            _check(lib().sassy_hip_search_hamming_reads(self._h, pp, pl, len(patterns), texts._handle(), k,
                                                        WITHOUT_TRACE if without_trace else 0, C.byref(out)))
            r = Result(out)
            return r if as_result else r.matches
        pp, pl, n_patterns, tp, tl, n_texts, on_device, _alive = self._marshal_many(patterns, texts)
        if on_device:
            raise SassyHipError("search_hamming_many takes host texts only")
        out = C.c_void_p()
        _check(lib().sassy_hip_search_hamming_many(self._h, pp, pl, n_patterns, tp, tl, n_texts, k, WITHOUT_TRACE if without_trace else 0,
                                                   C.byref(out)))
        r = Result(out)
        return r if as_result else r.matches

    def hamming_best_pattern(self, patterns, texts: Sequence, k: int):
        """Per text the best Hamming hit over all patterns and strands (sassy_hip_hamming_best_pattern): (cost uint8,
        pattern uint32, strand uint8, start uint64) arrays of n_texts entries -- of search_hamming_many's records of a text
        the smallest under (cost, pattern_idx, '+' before '-', text_start); NO_MATCH (255), 0xFFFFFFFF, 0 and
        0xFFFFFFFFFFFFFFFF where no pattern has a hit with at most k mismatches.  Reduced on the device: no records, no
        cigars.  k <= 254.  Demultiplexing by mismatch count."""
        import numpy as np
        patterns = self._hamming_patterns(patterns, "hamming_best_pattern")
        if isinstance(texts, DeviceReads):  # a resident read batch: sassy_hip_hamming_best_pattern_reads
            pp, pl = self._pattern_arrays(patterns)
            n = len(texts)
            cost, pattern = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint32)
            strand, start = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint64)
            _check(lib().sassy_hip_hamming_best_pattern_reads(self._h, pp, pl, len(patterns), texts._handle(), k, 0, cost.ctypes.data,
                                                              pattern.ctypes.data, strand.ctypes.data, start.ctypes.data))
            return cost, pattern, strand, start
        pp, pl, n_patterns, tp, tl, n_texts, on_device, _alive = self._marshal_many(patterns, texts)
        if on_device:
            raise SassyHipError("hamming_best_pattern takes host texts only")
        cost = np.empty(n_texts, dtype=np.uint8)
        pattern = np.empty(n_texts, dtype=np.uint32)
        strand = np.empty(n_texts, dtype=np.uint8)
        start = np.empty(n_texts, dtype=np.uint64)
        _check(lib().sassy_hip_hamming_best_pattern(self._h, pp, pl, n_patterns, tp, tl, n_texts, k, 0, cost.ctypes.data,
                                                    pattern.ctypes.data, strand.ctypes.data, start.ctypes.data))
        return cost, pattern, strand, start

    def hamming_counts(self, patterns, text, k: int):
        """How many hits `search_hamming(patterns, text, k)` has per pattern, strand and cost (sassy_hip_hamming_counts): a
        numpy.uint64 array of shape (n_patterns, 2, k + 1) -- [p, 0 '+' / 1 '-', c] --, counted on the device: no records are
        made.  The same searcher, so the same profile, rc and max_n_frac rule; the '-' rows of a searcher without rc are
        zero.  `text` as for `search_hamming` (a DeviceBuffer included; `text_unchanged()` is honoured).  k <= 254."""
        import numpy as np
        patterns = self._hamming_patterns(patterns, "hamming_counts")
        pp = (C.c_char_p * len(patterns))(*patterns)
        pl = (C.c_size_t * len(patterns))(*[len(p) for p in patterns])
        flags = 0
        addr, n, keep, on_dev = _ptr_len(text)
        if on_dev:
            flags |= TEXT_ON_DEVICE
            if getattr(self, "_text_unchanged", False):
                flags |= TEXT_UNCHANGED
        counts = np.zeros((len(patterns), 2, max(0, min(int(k), 254)) + 1), dtype=np.uint64)
        _check(lib().sassy_hip_hamming_counts(self._h, pp, pl, len(patterns), addr, n, k, flags, counts.ctypes.data))
        return counts

    def hamming_counts_many(self, patterns, texts: Sequence, k: int):
        """`hamming_counts` over a batch of texts, summed over all of them (sassy_hip_hamming_counts_many): the records of
        `search_hamming_many(patterns, texts, k)` counted per pattern, strand and cost, shape (n_patterns, 2, k + 1).
        `texts`: a list of host texts or a TextBatch (host texts only)."""
        import numpy as np
        patterns = self._hamming_patterns(patterns, "hamming_counts_many")
        if isinstance(texts, DeviceReads):  # a resident read batch: sassy_hip_hamming_counts_reads
            pp, pl = self._pattern_arrays(patterns)
            counts = np.zeros((len(patterns), 2, max(0, min(int(k), 254)) + 1), dtype=np.uint64)
            _check(lib().sassy_hip_hamming_counts_reads(self._h, pp, pl, len(patterns), texts._handle(), k, 0, counts.ctypes.data))
            return counts
        pp, pl, n_patterns, tp, tl, n_texts, on_device, _alive = self._marshal_many(patterns, texts)
        if on_device:
            raise SassyHipError("hamming_counts_many takes host texts only")
        counts = np.zeros((n_patterns, 2, max(0, min(int(k), 254)) + 1), dtype=np.uint64)
        _check(lib().sassy_hip_hamming_counts_many(self._h, pp, pl, n_patterns, tp, tl, n_texts, k, 0, counts.ctypes.data))
        return counts

    def hamming_amplicons(self, pairs, text, k: int, min_len: int, max_len: int):
        """Which products primer pairs make (in-silico PCR, sassy_hip_hamming_amplicons): a numpy structured array of
        `amplicon_dtype()` -- start, end, pair_idx, strand, fwd_cost, rev_cost -- ordered by (pair_idx, strand, start, end).
        `pairs`: a sequence of (fwd, rev) bytes, both written 5'->3'.  Strand 0: fwd matches at `start` and
        reverse_complement(rev) ends at `end`; strand 1 (an rc searcher only): rev at `start`, reverse_complement(fwd) at the
        end; each with at most k mismatches, min_len <= end - start <= max_len, and every such combination a record.  Joined
        on the device: no Hamming records are made.  `text` as for `search_hamming` (a DeviceBuffer included).  Dna and Iupac
        searchers, k <= 254, max_len <= 2^24."""
        import numpy as np
        pairs = [(bytes(f), bytes(r)) for f, r in pairs]
        n = len(pairs)
        fp = (C.c_char_p * max(1, n))(*[f for f, _ in pairs])
        fl = (C.c_size_t * max(1, n))(*[len(f) for f, _ in pairs])
        rp = (C.c_char_p * max(1, n))(*[r for _, r in pairs])
        rl = (C.c_size_t * max(1, n))(*[len(r) for _, r in pairs])
        flags = 0
        addr, tn, keep, on_dev = _ptr_len(text)
        if on_dev:
            flags |= TEXT_ON_DEVICE
            if getattr(self, "_text_unchanged", False):
                flags |= TEXT_UNCHANGED
        out, n_out = C.c_void_p(), C.c_size_t()
        _check(lib().sassy_hip_hamming_amplicons(self._h, fp, fl, rp, rl, n, addr, tn, k, min_len, max_len, flags, C.byref(out), C.byref(n_out)))
        dt = amplicon_dtype()
        if not n_out.value:
            return np.zeros(0, dtype=dt)
        try:
            return np.frombuffer(_bytes_at(out.value, n_out.value * dt.itemsize), dtype=dt).copy()
        finally:
            lib().sassy_hip_amplicons_free(out)

    @staticmethod
    def _pairs_lists(a, b, who: str, one_length: bool = True):
        a = pairs_sequences(a, who)
        if len(a) == 0:
            raise SassyHipError(f"{who} needs at least one sequence in a")
        if b is not None:
            b = pairs_sequences(b, who)
            if len(b) == 0:
                raise SassyHipError(f"{who}: b holds no sequence (b=None compares a with itself)")
            if one_length and b.shape[1] != a.shape[1]:
                raise SassyHipError(f"{who} takes sequences of one length: b has {b.shape[1]} bytes per sequence, a has {a.shape[1]}")
        return a, b

    def hamming_pairs(self, a, b=None, k: int = 0):
        """All-vs-all Hamming distances (sassy_hip_hamming_pairs): every (a_idx, b_idx, strand) with at most k mismatches
        between sequence a[a_idx] and b[b_idx] (strand 1, an rc searcher only: and reverse_complement(b[b_idx])) as a numpy
        structured array of `hamming_pair_dtype()`, ordered by (a_idx, b_idx, strand).  All sequences share one length
        m <= 128; `a`, `b`: a list of equal-length bytes or a C-contiguous uint8 array of shape (n, m).  b = None is self
        mode: every unordered pair of `a` once -- strand 0: a_idx < b_idx; strand 1: a_idx <= b_idx, (i, i, 1) included.
        Compared on the device as bit planes: no text, no records but the pairs.  k <= 254."""
        import numpy as np
        a, b = self._pairs_lists(a, b, "hamming_pairs")
        out, n_out = C.c_void_p(), C.c_size_t()
        _check(lib().sassy_hip_hamming_pairs(self._h, a.ctypes.data, len(a), None if b is None else b.ctypes.data,
                                             0 if b is None else len(b), a.shape[1], k, 0, C.byref(out), C.byref(n_out)))
        dt = hamming_pair_dtype()
        if not n_out.value:
            return np.zeros(0, dtype=dt)
        try:
            return np.frombuffer(_bytes_at(out.value, n_out.value * dt.itemsize), dtype=dt).copy()
        finally:
            lib().sassy_hip_hamming_pairs_free(out)

    def hamming_nearest(self, a, b=None, k: int = 0):
        """Per sequence of `a` its nearest sequence of `b` (sassy_hip_hamming_nearest): (cost uint8, index uint32, strand
        uint8, ties uint32) arrays of len(a) entries -- of the candidates (b_idx, strand) with at most k mismatches the
        smallest under (cost, b_idx, strand 0 before 1), and how many candidates share that cost (1: the correction is
        unambiguous); NO_MATCH (255), 0xFFFFFFFF, 0, 0 where there is none.  b = None: the nearest OTHER entry of `a` -- the
        full square, only (index == i, strand 0) is no candidate.  Inputs as for `hamming_pairs`.  k <= 254."""
        import numpy as np
        a, b = self._pairs_lists(a, b, "hamming_nearest")
        n = len(a)
        cost = np.empty(n, dtype=np.uint8)
        index = np.empty(n, dtype=np.uint32)
        strand = np.empty(n, dtype=np.uint8)
        ties = np.empty(n, dtype=np.uint32)
        _check(lib().sassy_hip_hamming_nearest(self._h, a.ctypes.data, n, None if b is None else b.ctypes.data,
                                               0 if b is None else len(b), a.shape[1], k, 0, cost.ctypes.data, index.ctypes.data,
                                               strand.ctypes.data, ties.ctypes.data))
        return cost, index, strand, ties

    def edit_pairs(self, a, b=None, k: int = 0):
        """All-vs-all edit distances (sassy_hip_edit_pairs): `hamming_pairs` with the Levenshtein distance E in place of
        H -- substitution, insertion and deletion cost 1 each and both sequences are consumed whole --, so a sequence that
        lost or gained a base is at cost 1 from its origin.  Every (a_idx, b_idx, strand) with E <= k as a structured
        array of `hamming_pair_dtype()`, ordered by (a_idx, b_idx, strand); strand 1 (an rc searcher only) is
        E(a, reverse_complement(b)).  The sequences of `a` share one length m_a <= 64 and those of `b` one length
        m_b <= 64; the two may differ (|m_a - m_b| > k: no record).  Inputs, self mode (b = None) and its triangle as for
        `hamming_pairs`.  k <= 254."""
        import numpy as np
        a, b = self._pairs_lists(a, b, "edit_pairs", one_length=False)
        out, n_out = C.c_void_p(), C.c_size_t()
        _check(lib().sassy_hip_edit_pairs(self._h, a.ctypes.data, len(a), a.shape[1], None if b is None else b.ctypes.data,
                                          0 if b is None else len(b), 0 if b is None else b.shape[1], k, 0, C.byref(out), C.byref(n_out)))
        dt = hamming_pair_dtype()
        if not n_out.value:
            return np.zeros(0, dtype=dt)
        try:
            return np.frombuffer(_bytes_at(out.value, n_out.value * dt.itemsize), dtype=dt).copy()
        finally:
            lib().sassy_hip_edit_pairs_free(out)

    def edit_nearest(self, a, b=None, k: int = 0):
        """Per sequence of `a` its nearest sequence of `b` under the edit distance (sassy_hip_edit_nearest): (cost uint8,
        index uint32, strand uint8, ties uint32) arrays exactly as `hamming_nearest` returns them, with E in place of H.
        Inputs as for `edit_pairs`.  k <= 254."""
        import numpy as np
        a, b = self._pairs_lists(a, b, "edit_nearest", one_length=False)
        n = len(a)
        cost = np.empty(n, dtype=np.uint8)
        index = np.empty(n, dtype=np.uint32)
        strand = np.empty(n, dtype=np.uint8)
        ties = np.empty(n, dtype=np.uint32)
        _check(lib().sassy_hip_edit_nearest(self._h, a.ctypes.data, n, a.shape[1], None if b is None else b.ctypes.data,
                                            0 if b is None else len(b), 0 if b is None else b.shape[1], k, 0, cost.ctypes.data,
                                            index.ctypes.data, strand.ctypes.data, ties.ctypes.data))
        return cost, index, strand, ties

    def _clusters(self, entry, a, k: int, who: str):
        import numpy as np
        a, _ = self._pairs_lists(a, None, who)
        n = len(a)
        labels = np.empty(n, dtype=np.uint32)
        sizes = np.empty(n, dtype=np.uint32)
        _check(entry(self._h, a.ctypes.data, n, a.shape[1], k, 0, labels.ctypes.data, sizes.ctypes.data, None))
        return labels, sizes

    def hamming_clusters(self, a, k: int = 0):
        """The groups a set of sequences forms (sassy_hip_hamming_clusters): the connected components of the graph with an
        edge between two sequences of `a` that are within k mismatches of each other (an rc searcher: or of each other's
        reverse complement) -- the self-mode records of `hamming_pairs`, never made.  Returns (labels, sizes), uint32 arrays
        of len(a) entries: labels[i] is the smallest index of i's component (so labels[i] == i marks one sequence per
        cluster, and the array is the same on every run), sizes[i] the size of that component.  One length m <= 128; `a` as
        for `hamming_pairs`.  k <= 254; k >= m is one cluster.  Components, not a UMI rule: two sequences that are far apart
        share a cluster where a chain of near ones joins them, and Iupac's N joins whatever it meets."""
        return self._clusters(lib().sassy_hip_hamming_clusters, a, k, "hamming_clusters")

    def edit_clusters(self, a, k: int = 0):
        """`hamming_clusters` under the edit distance (sassy_hip_edit_clusters): an edge where E <= k, so a sequence that lost
        or gained a base joins its origin at k = 1.  One length m <= 64.  Returns (labels, sizes) as `hamming_clusters`."""
        return self._clusters(lib().sassy_hip_edit_clusters, a, k, "edit_clusters")

    def umi_groups(self, a, k: int = 1, method: str = "directional"):
        """UMI grouping of a list of reads' UMIs (sassy_hip_umi_groups): identical sequences are counted and collapsed on the
        device, only the distinct ones are compared, and `method` makes the groups -- "unique": a group is a set of identical
        sequences (k is ignored); "cluster": the connected components within k mismatches, exactly `hamming_clusters`' labels
        and sizes; "directional": UMI-tools' rule -- a sequence of count c_u absorbs a neighbour of count c_v where
        c_u >= 2 c_v - 1, the sequences gone through by (count descending, first index ascending), so two abundant neighbours
        stay apart.  Returns (labels, sizes, reps, counts), uint32 arrays of len(a) entries: reps[i] the smallest index with
        i's sequence (reps[i] == i marks the distinct ones; what counts as identical is the pair calls' encoding: case folds
        under dna, iupac and ascii_ci, and Iupac's N is no duplicate of A), counts[i] how many reads carry it, labels[i] the
        first index of the sequence that opened i's group, sizes[i] the READS in that group.  The arrays are the same on every
        run.  One length m <= 128; `a` as for `hamming_pairs`; k <= 254."""
        import numpy as np
        if method not in UMI_METHODS:
            raise SassyHipError(f"umi_groups: method must be one of {', '.join(UMI_METHODS)} (got {method!r})")
        a, _ = self._pairs_lists(a, None, "umi_groups")
        n = len(a)
        labels, sizes, reps, counts = (np.empty(n, dtype=np.uint32) for _ in range(4))
        _check(lib().sassy_hip_umi_groups(self._h, a.ctypes.data, n, a.shape[1], k, UMI_METHODS[method], 0, labels.ctypes.data,
                                          sizes.ctypes.data, reps.ctypes.data, counts.ctypes.data, None, None))
        return labels, sizes, reps, counts

    def read_overlaps(self, r1, r2, min_overlap: int = 10, k: int = OVERLAP_MAX_LEN, max_permille: int = 200):
        """The best overlap of the two reads of every pair (sassy_hip_read_overlaps): pair r is read r of `r1` against the
        reverse complement of read r of `r2`, every end-to-end offset d (b[0] under a[d]) tried on the device.  An offset is
        accepted when it overlaps in at least `min_overlap` rows with at most `k` mismatches and at most `max_permille` per
        thousand of them; the best one has the lowest mismatch density, then the longer overlap, then the larger d.  Returns
        a numpy array of `read_overlap_dtype()` (offset, overlap, mismatches, n_accepted), all zero where nothing is accepted
        or a read is empty; `overlap_trims` derives insert length and trim points.  `r1` and `r2` are DeviceReads of equal
        length (reads of at most 512 bytes), or lists of byte sequences, which go through DeviceReads.from_sequences.  dna
        (A, C, G, T only) or iupac; the defaults accept up to 20 % mismatches and leave k open."""
        import numpy as np
        made = []
        # (lists: both are wrapped, and refused for a line end, before either is parsed)
        sources = [r if isinstance(r, DeviceReads) else fastq_from_sequences(r) for r in (r1, r2)]
        try:
            handles = []
            for r in sources:
                if not isinstance(r, DeviceReads):
                    r = DeviceReads(r)
                    made.append(r)
                handles.append(r)
            if not 0 <= int(min_overlap) < (1 << 32) or not 0 <= int(max_permille) < (1 << 32) or int(k) < 0:
                raise SassyHipError("read_overlaps: min_overlap, k and max_permille must not be negative")
            out = np.zeros(len(handles[0]), dtype=read_overlap_dtype())
            _check(lib().sassy_hip_read_overlaps(self._h, handles[0]._handle(), handles[1]._handle(), int(min_overlap), int(k), int(max_permille), 0,
                                                 out.ctypes.data if len(out) else None))
            return out
        finally:
            for r in made:
                r.free()

    def merge_pairs(self, r1, r2, min_overlap: int = 10, k: int = OVERLAP_MAX_LEN, max_permille: int = 200, with_overlaps: bool = False):
        """Every pair with an accepted overlap merged on the device (sassy_hip_merge_pairs): the overlap is `read_overlaps`'
        under the same `min_overlap`, `k`, `max_permille`; the merged read is a up to the overlap, the consensus inside it
        and b = reverse_complement(read of r2) behind it (a read-through pair: the overlap alone), with consensus qualities --
        equal bytes take the higher quality, different bytes the byte of the higher quality (a's on a tie) and
        min(126, 33 + max(2, |qa - qb|)).  Returns a new DeviceReads with kept qualities, ONE RECORD PER PAIR, empty where the
        pair was not merged, which every call that takes a DeviceReads takes; with `with_overlaps` also `read_overlaps`'
        array.  `r1`, `r2`: DeviceReads made with keep_quality=True, or lists of (sequence, quality) tuples.  The definition
        is tests/helpers/merge_pairs_ref.py."""
        import numpy as np
        made = []
        sources = [r if isinstance(r, DeviceReads) else fastq_from_sequences([x[0] for x in r], [x[1] for x in r]) for r in (r1, r2)]
        try:
            handles = []
            for r in sources:
                if not isinstance(r, DeviceReads):
                    r = DeviceReads(r, keep_quality=True)
                    made.append(r)
                handles.append(r)
            if not 0 <= int(min_overlap) < (1 << 32) or not 0 <= int(max_permille) < (1 << 32) or int(k) < 0:
                raise SassyHipError("merge_pairs: min_overlap, k and max_permille must not be negative")
            records = np.zeros(len(handles[0]), dtype=read_overlap_dtype()) if with_overlaps else None
            out = C.c_void_p()
            _check(lib().sassy_hip_merge_pairs(self._h, handles[0]._handle(), handles[1]._handle(), int(min_overlap), int(k), int(max_permille), 0,
                                               records.ctypes.data if with_overlaps and len(records) else None, C.byref(out)))
            merged = DeviceReads._adopt(out)
            return (merged, records) if with_overlaps else merged
        finally:
            for r in made:
                r.free()

    def search_all_alignments(self, pattern: bytes, text, k: int) -> List[List[Match]]:
        """Searcher::search_all_alignments (src/python.rs:117-135, src/search.rs:702-760): every alignment of cost <= k
        at every end position of search_all, grouped: one list per (strand, anchor) -- the anchor is text_end for
        Fwd matches and text_start for Rc matches --, Fwd groups by ascending text_end, then Rc groups by descending
        text_start, alignments in DFS order inside a group.  `text` as for `search` (bytes or a device tensor)."""
        pattern = _byte_pattern(pattern)
        addr, n, keep, on_dev = _ptr_len(text)
        flags = 0
        if on_dev:
            flags |= TEXT_ON_DEVICE
            if getattr(self, "_text_unchanged", False):
                flags |= TEXT_UNCHANGED
        out = C.c_void_p()
        _check(lib().sassy_hip_search_all_alignments(self._h, pattern, len(pattern), addr, n, k, flags, C.byref(out)))
        groups: List[List[Match]] = []
        last = None
        for x in Result(out).matches:
            key = (x.strand, x.text_end if x.strand == "+" else x.text_start)
            if key != last:
                groups.append([])
                last = key
            groups[-1].append(x)
        return groups

    def search_with_fn(self, pattern: bytes, text: bytes, k: int, all_minima: bool, filter_fn) -> List[Match]:
        """Searcher::search_with_fn (src/search.rs:767-784): keep the end positions for which
        filter_fn(pattern_of_strand: bytes, text_till_end: bytes, strand: '+'|'-') is true."""
        pattern, text = _byte_pattern(pattern), bytes(text)

        def tramp(p, plen, t, end, strand, _user):
            return 1 if filter_fn(C.string_at(p, plen), C.string_at(t, end), "-" if strand else "+") else 0

        cb = END_FILTER(tramp)
        out = C.c_void_p()
        addr = C.cast(C.c_char_p(text), C.c_void_p).value or 0
        _check(lib().sassy_hip_search_with_fn(self._h, pattern, len(pattern), addr, len(text), k,
                                              ALL_MINIMA if all_minima else 0, cb, None, C.byref(out)))
        return Result(out).matches

    @staticmethod
    def _marshal_many(patterns: Sequence[bytes], texts: Sequence):
        """(pattern pointers, pattern lengths, n_patterns, text pointers, text lengths, n_texts, texts on the device, what
        must stay alive during the call) for the many-pattern calls; `texts` a list or a TextBatch."""
        held = None
        patterns = [_byte_pattern(p) for p in patterns]
        pp = (C.c_char_p * len(patterns))(*patterns)
        pl = (C.c_size_t * len(patterns))(*[len(p) for p in patterns])
        if isinstance(texts, TextBatch):
            n_texts, on_device = len(texts), False
            tp = texts._addr.ctypes.data_as(C.POINTER(C.c_void_p))
            tl = texts.lens.ctypes.data_as(C.POINTER(C.c_size_t))
        elif _BYTES_PAYLOAD_OFFSET is not None and len(texts) and set(map(type, texts)) == {bytes}:
            # a read set: ctypes fills the pointer array from the list itself (a few hundred thousand _ptr_len calls
            # cost more than the search)
            import numpy as np
            n_texts, on_device = len(texts), False
            # (CPython: the bytes of a bytes object sit bytes.__basicsize__ - 1 behind its address, and an object
            # array IS the array of these addresses; `held` keeps the objects alive for the call)
            held = np.empty(n_texts, dtype=object)
            held[:] = texts
            addr = np.frombuffer((C.c_uint64 * n_texts).from_address(held.ctypes.data), dtype=np.uint64) + np.uint64(_BYTES_PAYLOAD_OFFSET)
            lens = np.fromiter(map(len, texts), dtype=np.uint64, count=n_texts)
            tp = addr.ctypes.data_as(C.POINTER(C.c_void_p))
            tl = lens.ctypes.data_as(C.POINTER(C.c_size_t))
            held = (held, addr, lens)
        else:
            infos = [_ptr_len(t) for t in texts]
            on_dev = [i[3] for i in infos]
            if any(on_dev) and not all(on_dev):
                raise SassyHipError("texts must be all on the host or all on the device")
            n_texts, on_device = len(infos), bool(infos and on_dev[0])
            tp = (C.c_void_p * n_texts)(*[i[0] for i in infos])
            tl = (C.c_size_t * n_texts)(*[i[1] for i in infos])
            held = infos
        return pp, pl, len(patterns), tp, tl, n_texts, on_device, (patterns, texts, held, tp, tl)

    @staticmethod
    def _marshal_patterns(patterns: Sequence[bytes]):
        """(pattern pointers, pattern lengths, n_patterns, what must stay alive) for the calls over a DeviceReads"""
        patterns = [_byte_pattern(p) for p in patterns]
        return (C.c_char_p * len(patterns))(*patterns), (C.c_size_t * len(patterns))(*[len(p) for p in patterns]), len(patterns), patterns

    def search_many(self, patterns: Sequence[bytes], texts: Sequence, k: int, all_minima: bool = False, as_result: bool = False,
                    without_trace: bool = False):
        """Searcher::search_many in SearchMode::Single order (src/search.rs:531-560): every pattern in
        every text, pattern-major; matches carry pattern_idx and text_idx.  as_result: the Result itself (numpy `.array`,
        `.lazy_matches`) instead of a list of Match objects.  `texts`: a list, a TextBatch, or a DeviceReads -- a read batch
        parsed on the device and laid out for the scan there, without a host layout or an upload (sassy_hip_search_many_reads;
        min_costs, best_pattern, best_matches and search_texts take one likewise)."""
        if isinstance(texts, DeviceReads):
            pp, pl, n_patterns, _alive = self._marshal_patterns(patterns)
            out = C.c_void_p()
            _check(lib().sassy_hip_search_many_reads(self._h, pp, pl, n_patterns, texts._handle(), k,
                                                     (ALL_MINIMA if all_minima else 0) | (WITHOUT_TRACE if without_trace else 0), C.byref(out)))
            r = Result(out)
            return r if as_result else r.matches
        pp, pl, n_patterns, tp, tl, n_texts, on_device, _alive = self._marshal_many(patterns, texts)
        flags = (ALL_MINIMA if all_minima else 0) | (TEXT_ON_DEVICE if on_device else 0) | (WITHOUT_TRACE if without_trace else 0)
        out = C.c_void_p()
        _check(lib().sassy_hip_search_many(self._h, pp, pl, n_patterns, tp, tl, n_texts, k, flags, C.byref(out)))
        r = Result(out)
        return r if as_result else r.matches

    def min_costs(self, patterns: Sequence[bytes], texts: Sequence, k: int, strands: bool = False):
        """The smallest cost of any match of pattern p in text t (what min(m.cost) over search_many's matches of the pair
        gives), NO_MATCH (255) where there is none of cost <= k: a numpy uint8 array (n_patterns, n_texts).  strands=True:
        (costs, strands) -- the strand of each minimum, 0 Fwd / 1 Rc, Fwd on a tie.  A batch of host texts is reduced on
        the device from the scan's own list: no records, no traceback.  `texts` a list or a TextBatch, as search_many."""
        import numpy as np
        if isinstance(texts, DeviceReads):  # a resident read batch: sassy_hip_min_costs_reads
            pp, pl, n_patterns, _alive = self._marshal_patterns(patterns)
            cost = np.empty((n_patterns, len(texts)), dtype=np.uint8)
            strand = np.empty((n_patterns, len(texts)), dtype=np.uint8) if strands else None
            _check(lib().sassy_hip_min_costs_reads(self._h, pp, pl, n_patterns, texts._handle(), k, 0, cost.ctypes.data,
                                                   strand.ctypes.data if strands else None))
            return (cost, strand) if strands else cost
        pp, pl, n_patterns, tp, tl, n_texts, on_device, _alive = self._marshal_many(patterns, texts)
        cost = np.empty((n_patterns, n_texts), dtype=np.uint8)
        strand = np.empty((n_patterns, n_texts), dtype=np.uint8) if strands else None
        _check(lib().sassy_hip_min_costs(self._h, pp, pl, n_patterns, tp, tl, n_texts, k, TEXT_ON_DEVICE if on_device else 0,
                                         cost.ctypes.data, strand.ctypes.data if strands else None))
        return (cost, strand) if strands else cost

    def best_pattern(self, patterns: Sequence[bytes], texts: Sequence, k: int):
        """Per text the best pattern: (cost uint8, pattern uint32, strand uint8) arrays of n_texts entries -- the smallest
        cost over all patterns and strands (NO_MATCH = 255: no match of cost <= k), the pattern that attains it (lowest
        index on a tie, then Fwd before Rc; 0xFFFFFFFF where there is no match) and its strand.  Demultiplexing, and
        `filter`: a record is kept when its cost is not NO_MATCH."""
        import numpy as np
        if isinstance(texts, DeviceReads):  # a resident read batch: sassy_hip_best_pattern_reads
            pp, pl, n_patterns, _alive = self._marshal_patterns(patterns)
            cost, pattern, strand = np.empty(len(texts), dtype=np.uint8), np.empty(len(texts), dtype=np.uint32), np.empty(len(texts), dtype=np.uint8)
            _check(lib().sassy_hip_best_pattern_reads(self._h, pp, pl, n_patterns, texts._handle(), k, 0, cost.ctypes.data, pattern.ctypes.data,
                                                      strand.ctypes.data))
            return cost, pattern, strand
        pp, pl, n_patterns, tp, tl, n_texts, on_device, _alive = self._marshal_many(patterns, texts)
        cost = np.empty(n_texts, dtype=np.uint8)
        pattern = np.empty(n_texts, dtype=np.uint32)
        strand = np.empty(n_texts, dtype=np.uint8)
        _check(lib().sassy_hip_best_pattern(self._h, pp, pl, n_patterns, tp, tl, n_texts, k, TEXT_ON_DEVICE if on_device else 0,
                                            cost.ctypes.data, pattern.ctypes.data, strand.ctypes.data))
        return cost, pattern, strand

    def best_matches(self, patterns: Sequence[bytes], texts: Sequence, k: int, as_result: bool = False, without_trace: bool = False):
        """Per text the one best match over all patterns and strands, as a complete record (where best_pattern says which
        pattern, this also says where): of search_many's records of a text -- only_best_match off -- the one with the
        lowest cost, then the lowest pattern_idx, then Fwd before Rc, then the rightmost end in the strand's scan
        direction (largest text_end for Fwd, smallest text_start for Rc).  At most one Match per text, ascending text_idx;
        a text without a match of cost <= k has none.  A batch of host texts is reduced and traced on the device: one
        traceback per text.  without_trace: end and cost only.  as_result: the Result itself.  `texts` a list or a
        TextBatch, as search_many, or a DeviceReads."""
        if isinstance(texts, DeviceReads):  # a resident read batch: sassy_hip_best_matches_reads
            pp, pl, n_patterns, _alive = self._marshal_patterns(patterns)
            out = C.c_void_p()
            _check(lib().sassy_hip_best_matches_reads(self._h, pp, pl, n_patterns, texts._handle(), k, WITHOUT_TRACE if without_trace else 0,
                                                      C.byref(out)))
            r = Result(out)
            return r if as_result else r.matches
        pp, pl, n_patterns, tp, tl, n_texts, on_device, _alive = self._marshal_many(patterns, texts)
        flags = (WITHOUT_TRACE if without_trace else 0) | (TEXT_ON_DEVICE if on_device else 0)
        out = C.c_void_p()
        _check(lib().sassy_hip_best_matches(self._h, pp, pl, n_patterns, tp, tl, n_texts, k, flags, C.byref(out)))
        r = Result(out)
        return r if as_result else r.matches

    def search_patterns(self, patterns: Sequence[bytes], text, k: int) -> List[Match]:
        """Searcher::search_patterns (src/search.rs:648-678): equal-length patterns in one text."""
        patterns = [_byte_pattern(p) for p in patterns]
        if patterns and any(len(p) != len(patterns[0]) for p in patterns):
            raise SassyHipError("All patterns passed to search_patterns must have the same length")
        return self.search_many(patterns, [text], k)

    def search_texts(self, pattern: bytes, texts: Sequence, k: int) -> List[Match]:
        """Searcher::search_texts (src/search.rs:615-637): one pattern in many texts."""
        return self.search_many([pattern], texts, k)

    def format_tsv(self, m: Match, pat_id: str, text_id: str, text: bytes, sam: bool = False) -> str:
        """One row of the reference CLI's match table (bin/grep.rs:710-757)."""
        cm = _HipMatch()
        cm.pattern_idx, cm.text_idx = m.pattern_idx, m.text_idx
        cm.text_start, cm.text_end = m.text_start, m.text_end
        cm.pattern_start, cm.pattern_end = m.pattern_start, m.pattern_end
        cm.cost, cm.strand = m.cost, 1 if m.strand == "-" else 0
        if isinstance(text, tuple):  # (address, length) of a text that lives in somebody's buffer (fastx.RecordBatch): no copy
            addr, tlen = int(text[0]), int(text[1])
        else:
            text = bytes(text)
            addr, tlen = C.cast(C.c_char_p(text), C.c_void_p).value or 0, len(text)
        args = (self._h, C.byref(cm), m.cigar.encode(), pat_id.encode(), text_id.encode(), addr, tlen, int(sam))
        need = lib().sassy_hip_format_tsv(*args, None, 0)
        if need < 0:
            raise SassyHipError(lib().sassy_hip_last_error().decode())
        buf = C.create_string_buffer(need + 1)
        lib().sassy_hip_format_tsv(*args, buf, need + 1)
        return buf.value.decode()

    def only_best_match(self, on: bool = True) -> "Searcher":
        """Searcher::only_best_match (src/search.rs:442-446)."""
        _check(lib().sassy_hip_set_only_best_match(self._h, int(on)))
        return self

    def with_max_overhang(self, max_overhang: Optional[int]) -> "Searcher":
        """Searcher::with_max_overhang (src/search.rs:436-440)."""
        _check(lib().sassy_hip_set_max_overhang(self._h, -1 if max_overhang is None else int(max_overhang)))
        return self

    def with_max_n_frac(self, max_n_frac: Optional[float]) -> "Searcher":
        """Searcher::with_max_n_frac / without_max_n_frac (src/search.rs:454-475)."""
        _check(lib().sassy_hip_set_max_n_frac(self._h, float("nan") if max_n_frac is None else float(max_n_frac)))
        return self

    def encode_patterns(self, patterns: Sequence[bytes]) -> EncodedPatterns:
        patterns = [_byte_pattern(p) for p in patterns]
        if not patterns:
            raise SassyHipError("No queries provided")
        plen = len(patterns[0])
        if any(len(p) != plen for p in patterns):
            raise SassyHipError("All pattern must have the same length")
        h = lib().sassy_hip_encode_patterns(self._h, b"".join(patterns), len(patterns), plen)
        if not h:
            raise SassyHipError(lib().sassy_hip_last_error().decode())
        return EncodedPatterns(h, len(patterns), plen)

    def search_encoded_patterns(self, encoded: EncodedPatterns, text, k: int,
                                all_minima: bool = False, as_result: bool = False, without_trace: bool = False):
        """Searcher::search_encoded_patterns (src/search.rs:415-423).  as_result: hand back the Result
        (numpy record array + cigar pool) instead of a list of Match objects -- for result sets with
        10^5 and more matches, where a Python object per match costs more than the search.
        without_trace: end positions and costs only (text_start = pattern_start = usize::MAX, empty cigar)."""
        addr, n, keep, on_dev = _ptr_len(text)
        out = C.c_void_p()
        flags = (ALL_MINIMA if all_minima else 0) | (TEXT_ON_DEVICE if on_dev else 0) | \
            (WITHOUT_TRACE if without_trace else 0)
        _check(lib().sassy_hip_search_encoded(self._h, encoded._h, addr, n, k, flags, C.byref(out)))
        r = Result(out)
        return r if as_result else r.matches

    # --- device-resident / multi-GPU entry points ---
    def search_shard(self, pattern: bytes, d_text_ptr: int, halo_len: int, shard_len: int,
                     global_offset: int, total_len: int, k: int, flags: int = 0) -> Result:
        out = C.c_void_p()
        pattern = _byte_pattern(pattern)
        _check(lib().sassy_hip_search_shard(self._h, pattern, len(pattern), d_text_ptr, halo_len,
                                            shard_len, global_offset, total_len, k, flags,
                                            C.byref(out)))
        return Result(out)

    def search_shard_begin(self, pattern: bytes, d_text_ptr: int, halo_len: int, shard_len: int,
                           global_offset: int, total_len: int, k: int, flags: int = 0) -> int:
        """Queue one search of a resident shard and return a ticket at once (sassy_hip_search_shard_begin);
        up to 2 may be in flight.  search_finish(ticket) waits for it and returns its Result."""
        out = C.c_void_p()
        pattern = _byte_pattern(pattern)
        _check(lib().sassy_hip_search_shard_begin(self._h, pattern, len(pattern), d_text_ptr, halo_len, shard_len,
                                                  global_offset, total_len, k, flags, C.byref(out)))
        return out.value

    def set_reference_lanes(self, lanes: int):
        """0 = the definition (default); 4 / 8 = the reports of the reference binary built for AVX2 / AVX-512."""
        _check(lib().sassy_hip_set_reference_lanes(self._h, int(lanes)))
        return self

    def set_geometry_tuner(self, on: bool = True):
        _check(lib().sassy_hip_set_geometry_tuner(self._h, int(on)))
        return self

    def set_pipe_depth(self, depth: int):
        _check(lib().sassy_hip_set_pipe_depth(self._h, int(depth)))
        return self

    def search_finish(self, ticket: int) -> Result:
        out = C.c_void_p()
        _check(lib().sassy_hip_search_finish(self._h, ticket, C.byref(out)))
        return Result(out)

    def set_stream(self, hip_stream_handle: int):
        _check(lib().sassy_hip_set_stream(self._h, hip_stream_handle or None))

    def set_timing(self, level: int):
        """0 = no HIP events, 1 = dominant kernel only (default), 2 = every phase."""
        _check(lib().sassy_hip_set_timing(self._h, int(level)))

    def set_prefilter(self, mode: int):
        """-1 = the library's choice, 0 = streaming DP over every block, 1 = prefilter also with short pieces."""
        _check(lib().sassy_hip_set_prefilter(self._h, int(mode)))
        return self

    def set_device(self, device: int):
        """Bind the searcher to a HIP device before its first search (default: the calling thread's current device)."""
        _check(lib().sassy_hip_set_device(self._h, int(device)))
        return self

    @property
    def device(self) -> int:
        return lib().sassy_hip_get_device(self._h)

    def set_fused(self, on: bool = True):
        """The bit-plane prefilter finishes the scan in its own launch (default) / always the classic kernel chain."""
        _check(lib().sassy_hip_set_fused(self._h, int(bool(on))))
        return self

    def set_option(self, name: str, value: int):
        """One entry of the searcher's switch table (csrc/switches.h): name in lower case without the SASSY_HIP_ prefix."""
        _check(lib().sassy_hip_set_option(self._h, name.encode(), int(value)))
        return self

    def get_option(self, name: str) -> int:
        v = C.c_long(0)
        _check(lib().sassy_hip_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def enable_counters(self, on: bool = True):
        _check(lib().sassy_hip_enable_counters(self._h, int(on)))

    def stats(self) -> dict:
        st = Stats()
        _check(lib().sassy_hip_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def text_unchanged(self, on: bool = True) -> "Searcher":
        """Promise that a device-resident text passed to the following searches holds the same bytes as
        in this searcher's previous call with that tensor (SASSY_HIP_TEXT_UNCHANGED): the reversed copy
        the Rc strand scans is then reused instead of rebuilt for every pattern."""
        self._text_unchanged = bool(on)
        return self

    def _search(self, pattern: bytes, text, k: int, flags: int) -> Result:
        pattern = _byte_pattern(pattern)
        addr, n, keep, on_dev = _ptr_len(text)
        if on_dev:
            flags |= TEXT_ON_DEVICE
            if getattr(self, "_text_unchanged", False):
                flags |= TEXT_UNCHANGED
        out = C.c_void_p()
        _check(lib().sassy_hip_search(self._h, pattern, len(pattern), addr, n, k, flags, C.byref(out)))
        return Result(out, flags)


def required_halo(pattern_len: int, k: int) -> int:
    return lib().sassy_hip_required_halo(pattern_len, k)


def merge_shards(results: Sequence["Result"], incoming_state: int = 1) -> "Result":
    """sassy_hip_merge_shards: the Results of consecutive shards (leftmost first) as one Result."""
    L = lib()
    hs = (C.c_void_p * len(results))(*[r._h for r in results])
    if any(h is None for h in hs):
        raise SassyHipError("merge_shards needs results that have not been materialised yet (their C records)")
    out = C.c_void_p()
    _check(L.sassy_hip_merge_shards(hs, len(results), int(incoming_state), C.byref(out)))
    return Result(out)


class MultiSearcher:
    """One text over several devices inside one process (include/sassy_hip.h: sassy_hip_multi_*): a shard and a host
    thread per entry of `devices` (None: every visible device; a device may be named more than once)."""

    def __init__(self, alphabet: str, devices: Optional[Sequence[int]] = None, alpha: float = float("nan")):
        L = lib()
        arr = (C.c_int * len(devices))(*devices) if devices else None
        self._h = L.sassy_hip_multi_new(alphabet.encode(), alpha, arr, len(devices) if devices else 0)
        if not self._h:
            raise SassyHipError(L.sassy_hip_last_error().decode())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().sassy_hip_multi_free(h)
            except Exception:
                pass

    @property
    def shards(self) -> int:
        return lib().sassy_hip_multi_shards(self._h)

    def devices(self) -> List[int]:
        return [lib().sassy_hip_multi_device(self._h, i) for i in range(self.shards)]

    def set_text(self, text: bytes, max_pattern_len: int, max_k: int):
        text = bytes(text)
        _check(lib().sassy_hip_multi_set_text(self._h, text, len(text), max_pattern_len, max_k))
        return self

    def generate_dna(self, n: int, seed: int, max_pattern_len: int, max_k: int):
        _check(lib().sassy_hip_multi_generate_dna(self._h, n, seed, max_pattern_len, max_k))
        return self

    def plant(self, seed: int, pattern: bytes, k: int, stride: int = 1 << 20) -> int:
        cnt = C.c_uint64()
        pattern = _byte_pattern(pattern)
        _check(lib().sassy_hip_multi_plant(self._h, seed, pattern, len(pattern), k, stride, C.byref(cnt)))
        return cnt.value

    def search(self, pattern: bytes, k: int, flags: int = 0) -> "Result":
        out = C.c_void_p()
        pattern = _byte_pattern(pattern)
        _check(lib().sassy_hip_multi_search(self._h, pattern, len(pattern), k, flags, C.byref(out)))
        return Result(out)

    def shard_stats(self, shard: int) -> dict:
        """Stats of the last search on one shard's searcher (sassy_hip_multi_searcher)."""
        st = Stats()
        h = lib().sassy_hip_multi_searcher(self._h, shard)
        if not h:
            raise SassyHipError("no such shard")
        _check(lib().sassy_hip_get_stats(h, C.byref(st)))
        return st.as_dict()

    def set_rc(self, rc: bool = True):
        """Both strands: searches append the Rc strand's matches (Searcher::new_rc)."""
        _check(lib().sassy_hip_multi_set_rc(self._h, int(bool(rc))))
        return self

    def set_replicated(self, on: bool = True):
        """Every device holds the whole text (before set_text / generate_dna): search_encoded shards the patterns."""
        _check(lib().sassy_hip_multi_set_replicated(self._h, int(bool(on))))
        return self

    def set_pipe_depth(self, depth: int) -> "MultiSearcher":
        _check(lib().sassy_hip_multi_set_pipe_depth(self._h, int(depth)))
        return self

    def search_begin(self, pattern: bytes, k: int, flags: int = 0) -> int:
        """Queues one search on every device and returns a ticket (sassy_hip_multi_search_begin)."""
        pattern = _byte_pattern(pattern)
        t = C.c_void_p()
        _check(lib().sassy_hip_multi_search_begin(self._h, pattern, len(pattern), k, flags, C.byref(t)))
        return t.value

    def search_finish(self, ticket: int) -> "Result":
        out = C.c_void_p()
        _check(lib().sassy_hip_multi_search_finish(self._h, ticket, C.byref(out)))
        return Result(out)

    def search_encoded(self, patterns: Sequence[bytes], k: int, flags: int = 0) -> "Result":
        patterns = [_byte_pattern(p) for p in patterns]
        if not patterns:
            raise SassyHipError("No queries provided")
        plen = len(patterns[0])
        if any(len(p) != plen for p in patterns):
            raise SassyHipError("All pattern must have the same length")
        out = C.c_void_p()
        _check(lib().sassy_hip_multi_search_encoded(self._h, b"".join(patterns), len(patterns), plen, k, flags, C.byref(out)))
        return Result(out)

    def search_many(self, patterns: Sequence[bytes], texts: Sequence[bytes], k: int, flags: int = 0) -> "Result":
        patterns = [_byte_pattern(p) for p in patterns]
        texts = [bytes(t) for t in texts]
        pp = (C.c_char_p * len(patterns))(*patterns)
        pl = (C.c_size_t * len(patterns))(*[len(p) for p in patterns])
        tp = (C.c_char_p * len(texts))(*texts)
        tl = (C.c_size_t * len(texts))(*[len(t) for t in texts])
        out = C.c_void_p()
        _check(lib().sassy_hip_multi_search_many(self._h, pp, pl, len(patterns), tp, tl, len(texts), k, flags, C.byref(out)))
        return Result(out)


def multi_layout(length: int, n_parts: int, max_pattern_len: int, max_k: int):
    """(parts that hold a share, [(offset, len, halo, halo_behind, rev_first, rev_end, rev_halo)] per part) -- the layout
    arithmetic of a MultiSearcher, no device needed (sassy_hip_multi_layout); -1 parts: a share is not covered."""
    out = (C.c_uint64 * (7 * n_parts))()
    e = lib().sassy_hip_multi_layout(length, n_parts, max_pattern_len, max_k, out)
    return e, [tuple(out[7 * i:7 * i + 7]) for i in range(n_parts)]


def seed_layout(alphabet: str, patterns: Sequence[bytes], k: int):
    """[(first row, rows)] of the k + 1 seeds the seeded search of search_encoded_patterns would use for these patterns
    (sassy_hip_seed_layout: host arithmetic, no device needed)."""
    patterns = [_byte_pattern(p) for p in patterns]
    if not patterns or any(len(p) != len(patterns[0]) for p in patterns):
        raise SassyHipError("seed_layout: patterns of one length, at least one")
    pp = (C.c_char_p * len(patterns))(*patterns)
    ends, lens = (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
    n = lib().sassy_hip_seed_layout(alphabet.encode(), pp, len(patterns), len(patterns[0]), k, ends, lens)
    if n < 0:
        raise SassyHipError("seed_layout: arguments out of range")
    return [(ends[i] - lens[i], lens[i]) for i in range(n)]


def seed_test_rows(pattern_len: int, k: int, seeds):
    """(win_left, largest offset, {piece: [(first row, rows, offset)]}) -- the sub-piece test's layout for the seeds
    [(first row, rows)] (sassy_hip_seed_test_rows: host arithmetic, no device needed); a piece without a test is left out."""
    ends = (C.c_uint32 * 8)(*[a + ln for a, ln in seeds])
    lens = (C.c_uint32 * 8)(*[ln for _, ln in seeds])
    rows, win = (C.c_uint32 * 64)(), C.c_uint32()
    mx = lib().sassy_hip_seed_test_rows(pattern_len, k, ends, lens, rows, C.byref(win))
    if mx < 0:
        raise SassyHipError("seed_test_rows: arguments out of range")
    out = {}
    for p in range(k + 1):
        if (rows[8 * p] & 0xFF) == 0xFF:
            continue
        out[p] = [((r & 0xFF) // 2, (32 - ((r >> 8) & 0xFF)) // 2, ((r >> 16) & 0xFF) // 2 + 16 * (r >> 24))
                  for r in (rows[8 * p + u] for u in range(k + 1))]
    return win.value, mx, out


def generate_dna(d_ptr: int, n: int, seed: int, first: int = 0, stream: int = 0):
    """Fill device memory [d_ptr, d_ptr+n) with the synthetic ACGT text."""
    _check(lib().sassy_hip_generate_dna(d_ptr, n, seed, first, stream or None))


def generate_genome_like(d_ptr: int, n: int, seed: int, first: int = 0, with_n: bool = False, stream: int = 0):
    """Fill device memory with the repeat-rich synthetic text (microsatellites, repeat families, optional N runs)."""
    _check(lib().sassy_hip_generate_genome_like(d_ptr, n, seed, first, int(with_n), stream or None))


def plant(d_ptr: int, n: int, first: int, total_n: int, seed: int, pattern: bytes, k: int,
          stride: int = 1 << 20, stream: int = 0, phase: int = 0) -> int:
    cnt = C.c_uint64()
    pattern = _byte_pattern(pattern)
    _check(lib().sassy_hip_plant_phase(d_ptr, n, first, total_n, seed, pattern, len(pattern), k, stride, phase,
                                       stream or None, C.byref(cnt)))
    return cnt.value


class DeviceBuffer:
    """hipMalloc'ed bytes for callers without torch (tests, C-style use)."""

    def __init__(self, nbytes: int):
        self.nbytes = nbytes
        self.ptr = lib().sassy_hip_malloc(nbytes)
        if not self.ptr:
            raise SassyHipError(lib().sassy_hip_last_error().decode())

    def upload(self, data: bytes, offset: int = 0):
        _check(lib().sassy_hip_memcpy_h2d(self.ptr + offset, data, len(data)))

    def download_into(self, array, offset: int = 0):
        """Device bytes [offset, offset + array.nbytes) into a writable numpy array (no intermediate copy)."""
        _check(lib().sassy_hip_memcpy_d2h(array.ctypes.data, self.ptr + offset, array.nbytes))
        return array

    def download(self, nbytes: Optional[int] = None, offset: int = 0) -> bytes:
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        buf = C.create_string_buffer(nbytes)
        _check(lib().sassy_hip_memcpy_d2h(buf, self.ptr + offset, nbytes))
        return buf.raw

    def free(self):
        if self.ptr:
            lib().sassy_hip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        self.free()


class DeviceText:
    """`nbytes` device-resident bytes at `ptr` as a `text` argument: the parts of a device tensor the searcher reads (data_ptr,
    numel, is_cuda, a 1-byte dtype).  The pointer is 16-byte aligned and readable up to the next multiple of 64 behind the
    text (SASSY_HIP_TEXT_ON_DEVICE); `owner` is whatever keeps the memory alive."""

    class _Byte:
        itemsize = 1

    dtype = _Byte()
    is_cuda = True

    def __init__(self, ptr: int, nbytes: int, owner=None):
        self._p, self._n, self._owner = int(ptr or 0), int(nbytes), owner

    def data_ptr(self) -> int:
        return self._p

    def numel(self) -> int:
        return self._n

    def is_contiguous(self) -> bool:
        return True

    def download(self) -> bytes:
        if not self._n:
            return b""
        buf = C.create_string_buffer(self._n)
        _check(lib().sassy_hip_memcpy_d2h(buf, self._p, self._n))
        return buf.raw


class DeviceFasta:
    """A chunk of FASTA unwrapped on the device (sassy_hip_fasta_unwrap): `raw` -- bytes, a numpy uint8 array, or a device
    text (DeviceText, a torch tensor) -- holds whole records and is empty or begins with '>'.  Headers and line ends are
    dropped by kernels; record i's sequence is `text(i)`, a device view that every `text` argument accepting device texts
    takes without a copy; only the record table comes back: `id_starts` / `id_lens` index `raw`, `seq_starts` (multiples of
    64) / `seq_lens` the device buffer.  The definition is the line-by-line parse (tests/helpers/fasta_ref.py)."""

    def __init__(self, raw, stream: int = 0):
        import numpy as np
        addr, n, keep, on_dev = _ptr_len(raw)
        self._raw, self._raw_on_device = keep, on_dev
        self._h = None
        out = C.c_void_p()
        _check(lib().sassy_hip_fasta_unwrap(addr, n, TEXT_ON_DEVICE if on_dev else 0, stream or None, C.byref(out)))
        self._h = out
        count = int(lib().sassy_hip_fasta_n_records(out))
        dt = fasta_record_dtype()
        table = (np.frombuffer(_bytes_at(lib().sassy_hip_fasta_records(out), count * dt.itemsize), dtype=dt) if count
                 else np.zeros(0, dtype=dt))
        self.id_starts, self.id_lens = table["id_start"].copy(), table["id_len"].copy()
        self.seq_starts, self.seq_lens = table["seq_start"].copy(), table["seq_len"].copy()
        self.ptr = int(lib().sassy_hip_fasta_text(out) or 0)
        self.text_bytes = int(lib().sassy_hip_fasta_text_bytes(out))

    def __len__(self) -> int:
        return len(self.id_starts)

    def _live(self):
        if self._h is None:
            raise SassyHipError("DeviceFasta: freed")

    def id(self, i: int) -> str:
        a, n = int(self.id_starts[i]), int(self.id_lens[i])
        if self._raw is None:
            raise SassyHipError("DeviceFasta: the raw bytes were let go (the ids are with whoever released them)")
        if self._raw_on_device:
            return DeviceText(self._raw.data_ptr() + a, n).download().decode()
        if isinstance(self._raw, bytes):
            return self._raw[a:a + n].decode()
        return self._raw[a:a + n].tobytes().decode()

    def text(self, i: int) -> DeviceText:
        """Record i's sequence on the device."""
        self._live()
        return DeviceText(self.ptr + int(self.seq_starts[i]), int(self.seq_lens[i]), owner=self)

    def download(self, i: int, start: int = 0, end: Optional[int] = None) -> bytes:
        """Record i's sequence, or its bytes [start, end), on the host."""
        self._live()
        n = int(self.seq_lens[i])
        end = n if end is None else min(int(end), n)
        start = max(0, int(start))
        if end <= start:
            return b""
        return DeviceText(self.ptr + int(self.seq_starts[i]) + start, end - start).download()

    def free(self):
        if getattr(self, "_h", None) is not None:
            try:
                lib().sassy_hip_fasta_free(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None
            self.ptr = 0

    def __del__(self):
        self.free()


class DeviceReads:
    """A chunk of FASTQ parsed on the device (sassy_hip_fastq_parse): `raw` -- bytes, a numpy uint8 array, or a device text
    (DeviceText, a torch tensor) -- holds whole records of strict four-line FASTQ and is empty or begins with '@'.  The
    sequences stay on the device in the layout the Hamming batch kernels scan: `search_hamming_many`, `hamming_best_pattern`
    and `hamming_counts_many` take the object as `texts`, any number of times, without an upload.  Only the record table
    comes back: `id_starts` / `id_lens` and `qual_starts` / `qual_lens` index `raw`, `seq_starts` (multiples of 64) /
    `seq_lens` the device buffer.  Malformed input raises SassyHipError and names the first bad record.  The definition is
    tests/helpers/fastq_ref.py."""

    def __init__(self, raw, stream: int = 0, keep_quality: bool = False):
        addr, n, keep, on_dev = _ptr_len(raw)
        self._raw, self._raw_on_device, self._adopted = keep, on_dev, False
        self._h = None
        out = C.c_void_p()
        _check(lib().sassy_hip_fastq_parse(addr, n, (TEXT_ON_DEVICE if on_dev else 0) | (KEEP_QUALITY if keep_quality else 0), stream or None,
                                           C.byref(out)))
        self._take(out)

    @classmethod
    def _adopt(cls, handle):
        """A handle that another call made (Searcher.merge_pairs): no raw bytes, so no ids; the qualities are on the device."""
        self = cls.__new__(cls)
        self._raw, self._raw_on_device, self._adopted = None, False, True
        self._take(handle)
        return self

    def _take(self, out):
        import numpy as np
        self._h = out
        count = int(lib().sassy_hip_reads_n(out))
        dt = read_record_dtype()
        # (a view of the handle's own table: the columns below are its only copy -- millions of reads are 48 bytes each)
        table = (np.frombuffer((C.c_char * (count * dt.itemsize)).from_address(lib().sassy_hip_reads_records(out)), dtype=dt) if count
                 else np.zeros(0, dtype=dt))
        self.id_starts, self.id_lens = table["id_start"].copy(), table["id_len"].copy()
        self.seq_starts, self.seq_lens = table["seq_start"].copy(), table["seq_len"].copy()
        self.qual_starts, self.qual_lens = table["qual_start"].copy(), table["qual_len"].copy()
        self.ptr = int(lib().sassy_hip_reads_text(out) or 0)
        self.text_bytes = int(lib().sassy_hip_reads_text_bytes(out))
        self.longest = int(lib().sassy_hip_reads_longest(out))
        self.qual_ptr = int(lib().sassy_hip_reads_quality(out) or 0)  # 0: the qualities were not kept

    @classmethod
    def from_sequences(cls, seqs, quals=None, stream: int = 0, keep_quality: Optional[bool] = None):
        """A read batch of a list of byte sequences: they are wrapped into minimal four-line FASTQ (fastq_from_sequences: an
        empty id and an empty quality each) and parsed like any chunk.  A sequence that holds '\\n' or '\\r' is refused.
        `quals`: a list of as many qualities of equal lengths; they are kept on the device unless keep_quality=False."""
        return cls(fastq_from_sequences(seqs, quals), stream, keep_quality=(quals is not None) if keep_quality is None else keep_quality)

    def __len__(self) -> int:
        return len(self.id_starts)

    def _live(self):
        if self._h is None:
            raise SassyHipError("DeviceReads: freed")

    def _handle(self):
        self._live()
        return self._h

    def _raw_bytes(self, a: int, n: int) -> bytes:
        if self._raw is None:
            raise SassyHipError("DeviceReads: the raw bytes were let go (ids and qualities are with whoever released them)")
        if self._raw_on_device:
            return DeviceText(self._raw.data_ptr() + a, n).download()
        if isinstance(self._raw, bytes):
            return self._raw[a:a + n]
        return self._raw[a:a + n].tobytes()

    def id(self, i: int) -> str:
        if self._adopted:
            raise SassyHipError("DeviceReads: a merged batch has no ids of its own: record r is pair r, and the ids are R1's")
        return self._raw_bytes(int(self.id_starts[i]), int(self.id_lens[i])).decode()

    def quality(self, i: int) -> bytes:
        """Read i's quality: from the device buffer where the handle keeps one, else out of the raw bytes."""
        if self.qual_ptr:
            self._live()
            n = int(self.seq_lens[i])
            return DeviceText(self.qual_ptr + int(self.seq_starts[i]), n).download() if n else b""
        return self._raw_bytes(int(self.qual_starts[i]), int(self.qual_lens[i]))

    def download_quality_text(self) -> bytes:
        """The whole quality buffer, the twin of download_text: the text's layout, pads and the 64 spare bytes included."""
        self._live()
        if not self.qual_ptr:
            raise SassyHipError("DeviceReads: the qualities were not kept (keep_quality=True keeps them on the device)")
        return DeviceText(self.qual_ptr, self.text_bytes).download()

    def text(self, i: int) -> DeviceText:
        """Read i's sequence on the device."""
        self._live()
        return DeviceText(self.ptr + int(self.seq_starts[i]), int(self.seq_lens[i]), owner=self)

    def download(self, i: int, start: int = 0, end: Optional[int] = None) -> bytes:
        """Read i's sequence, or its bytes [start, end), on the host."""
        self._live()
        n = int(self.seq_lens[i])
        end = n if end is None else min(int(end), n)
        start = max(0, int(start))
        if end <= start:
            return b""
        return DeviceText(self.ptr + int(self.seq_starts[i]) + start, end - start).download()

    def slice(self, begins, lens, stream: int = 0):
        """A new DeviceReads whose read r is bytes [begins[r], begins[r] + lens[r]) of this batch's read r, and of its quality
        where kept (sassy_hip_reads_slice): fixed clipping, a leading UMI or barcode split off.  `begins`, `lens`: one entry
        per read, or one number for all.  A window that reaches outside its read is refused."""
        import numpy as np
        self._live()
        n = len(self)
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(begins, dtype=np.uint64), (n,)))
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(lens, dtype=np.uint64), (n,)))
        out = C.c_void_p()
        _check(lib().sassy_hip_reads_slice(self._h, b.ctypes.data if n else None, w.ctypes.data if n else None, stream or None, C.byref(out)))
        return DeviceReads._adopt(out)

    def select(self, src, begins=None, lens=None, stream: int = 0):
        """A new DeviceReads whose record j is bytes [begins[j], begins[j] + lens[j]) of this batch's read src[j], and of its
        quality where kept (sassy_hip_reads_select); without `begins` and `lens`, whole reads.  `src` may repeat, skip and
        reorder: it takes one sample out of a demultiplexed batch, puts a mate batch into the order of another, drops empty
        records.  `begins`, `lens`: one entry per output record, or one number for all.  An index that names no read, or a
        window that reaches outside its read, is refused."""
        import numpy as np
        self._live()
        if (begins is None) != (lens is None):
            raise SassyHipError("select: begins and lens are given together, or neither (whole reads)")
        src = np.ascontiguousarray(np.asarray(src, dtype=np.uint64).reshape(-1))
        n = len(src)
        b = w = None
        if begins is not None:
            b = np.ascontiguousarray(np.broadcast_to(np.asarray(begins, dtype=np.uint64), (n,)))
            w = np.ascontiguousarray(np.broadcast_to(np.asarray(lens, dtype=np.uint64), (n,)))
            if n == 0:  # (the pair is still given together)
                b = w = np.zeros(1, dtype=np.uint64)
        out = C.c_void_p()
        _check(lib().sassy_hip_reads_select(self._h, src.ctypes.data if n else None, None if b is None else b.ctypes.data,
                                            None if w is None else w.ctypes.data, n, stream or None, C.byref(out)))
        return DeviceReads._adopt(out)

    def nonempty(self, stream: int = 0):
        """(reads, kept_indices): the records that hold a byte, in their order, as a new DeviceReads (a `select`), and which
        they were -- what drops the empty records a trim or a merge leaves."""
        import numpy as np
        kept = np.flatnonzero(self.seq_lens).astype(np.uint64)
        return self.select(kept, stream=stream), kept

    def demux(self, searcher, barcodes, k: int = 1, min_delta: int = 1, at: int = 0, end3: bool = False, clip: bool = True,
              with_records: bool = False):
        """The batch split by sample barcode on the device (sassy_hip_demux_reads).  `barcodes`: 1 .. 4096 byte strings of ONE
        length 1 .. 64.  A read's window is the barcode's length of bytes at distance `at` from its 5' end (`end3`: from its
        3' end); a read is assigned to the barcode of the fewest mismatches (the smaller index among equals) when that cost
        is at most `k` and the runner-up costs at least `min_delta` more.  Returns a `Demuxed`: `.reads` is a new DeviceReads
        SORTED BY SAMPLE, the unassigned last, assigned reads without their barcode (and without what lies between it and
        the read's end) unless clip=False; `.order[j]` is the read behind record j; sample s is the records
        [bounds[s], bounds[s + 1]).  `searcher`: dna (A, C, G, T only) or iupac; it runs the call on its stream and keeps the
        stats.  The definition is tests/helpers/demux_reads_ref.py."""
        import numpy as np
        self._live()
        barcodes = [b.encode() if isinstance(b, str) else _byte_pattern(b) for b in barcodes]
        if any(len(b) != len(barcodes[0]) for b in barcodes):
            raise SassyHipError("demux: the barcodes must all have one length")
        if any(not 0 <= int(v) < (1 << 32) for v in (min_delta, at)) or int(k) < 0:
            raise SassyHipError("demux: min_delta and at must fit 32 bits, and none of them nor k may be negative")
        n, nb = len(self), len(barcodes)
        ptrs = (C.c_char_p * max(nb, 1))(*barcodes)
        records = np.zeros(n, dtype=read_demux_dtype()) if with_records else None
        order = np.zeros(n, dtype=np.uint64)
        bounds = np.zeros(nb + 2, dtype=np.uint64)
        out = C.c_void_p()
        _check(lib().sassy_hip_demux_reads(searcher._h, self._h, ptrs, len(barcodes[0]) if nb else 0, nb, int(at), int(k), int(min_delta),
                                           (DEMUX_END3 if end3 else 0) | (0 if clip else DEMUX_KEEP_BARCODE),
                                           records.ctypes.data if with_records and n else None, order.ctypes.data if n else None,
                                           bounds.ctypes.data, C.byref(out)))
        return Demuxed(DeviceReads._adopt(out), order, bounds, records)

    def _dedup_args(self, who, umi_len, k, method, at):
        if method not in UMI_METHODS:
            raise SassyHipError(f"{who}: method must be one of {', '.join(UMI_METHODS)} (got {method!r})")
        if any(not 0 <= int(v) < (1 << 32) for v in (umi_len, at)) or int(k) < 0:
            raise SassyHipError(f"{who}: umi_len and at must fit 32 bits, and none of them nor k may be negative")

    def umi_groups(self, searcher, umi_len: int, k: int = 1, method: str = "directional", at: int = 0, end3: bool = False):
        """UMI grouping of the batch on the device (sassy_hip_umi_groups_reads): the key of a read is its window of `umi_len`
        bytes (1 .. 128) at distance `at` from its 5' end (`end3`: from its 3' end), and the groups are exactly what
        `Searcher.umi_groups` makes of the list of windows under the same searcher, k and method, with every index mapped back
        to its read.  Returns (label, size, rep, count, n_unique, n_groups): four uint32 arrays of len(self) entries and two
        numbers.  A read too short for a window takes no part: label = rep = 2^32 - 1, size = count = 0.  `searcher`: dna
        (A, C, G, T only) or iupac; rc=True groups across both strands.  The definition is tests/helpers/dedup_reads_ref.py."""
        import numpy as np
        self._live()
        self._dedup_args("umi_groups", umi_len, k, method, at)
        n = len(self)
        label, size, rep, count = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(4))
        n_unique, n_groups = C.c_size_t(0), C.c_size_t(0)
        _check(lib().sassy_hip_umi_groups_reads(searcher._h, self._h, int(at), int(umi_len), int(k), UMI_METHODS[method], DEDUP_END3 if end3 else 0,
                                                label.ctypes.data, size.ctypes.data, rep.ctypes.data, count.ctypes.data, C.byref(n_unique),
                                                C.byref(n_groups)))
        return label[:n], size[:n], rep[:n], count[:n], int(n_unique.value), int(n_groups.value)

    def dedup(self, searcher, umi_len: int, k: int = 1, method: str = "directional", at: int = 0, end3: bool = False, with_columns: bool = False):
        """The batch deduplicated by UMI on the device (sassy_hip_dedup_reads): the groups of `umi_groups`, and of every group
        the read with the highest score kept -- the sum of its quality bytes where the batch keeps qualities, else its
        length; on a tie the smallest index.  Returns a `Deduped`: `.reads` is a new DeviceReads whose record j is read
        `.kept[j]` whole (ascending), `.n_unique`, `.n_groups`, and with_columns=True `.label`, `.size`, `.rep`, `.count` as
        `umi_groups` returns them.  Clip the key off afterwards with `slice`.  The definition is
        tests/helpers/dedup_reads_ref.py."""
        import numpy as np
        self._live()
        self._dedup_args("dedup", umi_len, k, method, at)
        n = len(self)
        cols = tuple(np.zeros(n, dtype=np.uint32) for _ in range(4)) if with_columns else None
        ptr = lambda i: cols[i].ctypes.data if with_columns and n else None
        kept = np.zeros(max(n, 1), dtype=np.uint64)
        n_unique, n_groups = C.c_size_t(0), C.c_size_t(0)
        out = C.c_void_p()
        _check(lib().sassy_hip_dedup_reads(searcher._h, self._h, int(at), int(umi_len), int(k), UMI_METHODS[method], DEDUP_END3 if end3 else 0,
                                           ptr(0), ptr(1), ptr(2), ptr(3), kept.ctypes.data, C.byref(n_unique), C.byref(n_groups), C.byref(out)))
        return Deduped(DeviceReads._adopt(out), kept[:int(n_groups.value)].copy(), int(n_unique.value), int(n_groups.value), cols)

    def download_text(self) -> bytes:
        """The whole device buffer: the layout, pads and the 64 spare bytes included."""
        self._live()
        return DeviceText(self.ptr, self.text_bytes).download()

    def download_rem(self):
        """The per-block table the scan masks by (bytes left in the block's own read), as a numpy uint32 array."""
        import numpy as np
        self._live()
        n_blocks = (self.text_bytes - 64) // 64
        raw = DeviceText(int(lib().sassy_hip_reads_rem(self._h) or 0), 4 * n_blocks).download()
        return np.frombuffer(raw, dtype=np.uint32).copy()

    def free(self):
        if getattr(self, "_h", None) is not None:
            try:
                lib().sassy_hip_reads_free(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None
            self.ptr = 0
            self.qual_ptr = 0

    def __del__(self):
        self.free()


class Demuxed:
    """What `DeviceReads.demux` returns: `.reads`, the batch sorted by sample (the unassigned last); `.order`, per record of it
    the read of the input it was; `.bounds`, B + 2 places -- sample s is the records [bounds[s], bounds[s + 1]), the unassigned
    are [bounds[B], bounds[B + 1]); `.records`, one `read_demux_dtype()` per INPUT read where asked for, else None."""

    def __init__(self, reads, order, bounds, records=None):
        self.reads, self.order, self.bounds, self.records = reads, order, bounds, records

    @property
    def n_samples(self) -> int:
        return len(self.bounds) - 2

    @property
    def counts(self):
        """Reads per sample as a numpy array of B + 1 entries, the unassigned last."""
        import numpy as np
        return np.diff(self.bounds.astype(np.int64))

    def span(self, s: int):
        """(first, end) of sample s among the records of `.reads`; s = -1: the unassigned."""
        s = self.n_samples if s == -1 else int(s)
        if not 0 <= s <= self.n_samples:
            raise SassyHipError(f"Demuxed: sample {s} of {self.n_samples}")
        return int(self.bounds[s]), int(self.bounds[s + 1])

    def sample(self, s: int, stream: int = 0):
        """Sample s as a DeviceReads of its own (a `select` of its range); s = -1: the unassigned."""
        import numpy as np
        a, b = self.span(s)
        return self.reads.select(np.arange(a, b, dtype=np.uint64), stream=stream)

    def free(self):
        self.reads.free()


class Deduped:
    """What `DeviceReads.dedup` returns: `.reads`, the kept reads as a new DeviceReads; `.kept`, per record of it the read of
    the input it is (ascending); `.n_unique`, the distinct keys; `.n_groups`, the groups (= len(kept)); `.label`, `.size`,
    `.rep`, `.count`, one entry per INPUT read where asked for, else None."""

    def __init__(self, reads, kept, n_unique, n_groups, columns=None):
        self.reads, self.kept, self.n_unique, self.n_groups = reads, kept, n_unique, n_groups
        self.label, self.size, self.rep, self.count = columns if columns is not None else (None, None, None, None)

    def free(self):
        self.reads.free()


def _as_device_reads(reads):
    """(reads as a DeviceReads, the one made here or None)"""
    if isinstance(reads, DeviceReads):
        return reads, None
    reads = list(reads)
    paired = bool(reads) and isinstance(reads[0], tuple)
    made = DeviceReads.from_sequences([x[0] for x in reads], [x[1] for x in reads]) if paired else DeviceReads.from_sequences(reads)
    return made, made


def dedup_reads(searcher, reads, umi_len: int, k: int = 1, method: str = "directional", at: int = 0, end3: bool = False, with_columns: bool = False):
    """`DeviceReads.dedup` for a DeviceReads, or for a list of sequences or of (sequence, quality) tuples, which goes through
    `DeviceReads.from_sequences` first."""
    reads, made = _as_device_reads(reads)
    try:
        return reads.dedup(searcher, umi_len, k=k, method=method, at=at, end3=end3, with_columns=with_columns)
    finally:
        if made is not None:
            made.free()


def demux_reads(searcher, reads, barcodes, k: int = 1, min_delta: int = 1, at: int = 0, end3: bool = False, clip: bool = True,
                with_records: bool = False):
    """`DeviceReads.demux` for a DeviceReads, or for a list of sequences or of (sequence, quality) tuples, which goes through
    `DeviceReads.from_sequences` first."""
    made = None
    if not isinstance(reads, DeviceReads):
        reads = list(reads)
        paired = bool(reads) and isinstance(reads[0], tuple)
        made = reads = DeviceReads.from_sequences([x[0] for x in reads], [x[1] for x in reads]) if paired else DeviceReads.from_sequences(reads)
    try:
        return reads.demux(searcher, barcodes, k=k, min_delta=min_delta, at=at, end3=end3, clip=clip, with_records=with_records)
    finally:
        if made is not None:
            made.free()
