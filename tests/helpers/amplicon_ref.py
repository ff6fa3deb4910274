"""The amplicon join restated in Python, on top of tests/helpers/hamming_ref.py: per pair the Hamming records of [F, R] on both
strands (hamming_ref.expected(..., rc=True, without_trace=True)) and, per orientation, every (left site, right site) whose
span passes the definition's three conditions.  Shares nothing with the library.

  strand 0: left = F on '+' at start, right = R on '-' (reverse_complement(R) in the forward text) ending at end
  strand 1: left = R on '+' at start, right = F on '-' ending at end            (rc searchers only)
  min_len <= end - start <= max_len and end - start >= max(len(F), len(R))
"""
import bisect

import numpy as np

import hamming_ref as href

DTYPE = np.dtype([("start", "<u8"), ("end", "<u8"), ("pair_idx", "<u4"), ("strand", "u1"), ("fwd_cost", "u1"), ("rev_cost", "u1"),
                  ("pad_", "u1")])
FIELDS = ("start", "end", "pair_idx", "strand", "fwd_cost", "rev_cost", "pad_")


def join(hits, i, a, b, min_len, max_len, rc):
    """The records of pair i from `hits`, objects with pattern_idx (0: F, 1: R), strand ('+' / '-'), text_start and cost, in
    the order (strand, start, end)."""
    site = {(p, st): [] for p in (0, 1) for st in "+-"}
    for h in hits:
        site[(h.pattern_idx, h.strand)].append((h.text_start, h.cost))
    rows = []
    for strand in (0, 1) if rc else (0,):
        left = sorted(site[(0, "+")] if strand == 0 else site[(1, "+")])
        right = sorted(site[(1, "-")] if strand == 0 else site[(0, "-")])
        width = b if strand == 0 else a  # of the right site
        starts = [p for p, _ in right]
        for s, left_cost in left:
            # only right sites that start in [s - width, s + max_len] can pass; the definition decides
            for p, right_cost in right[bisect.bisect_left(starts, s - width):bisect.bisect_right(starts, s + max_len)]:
                end = p + width
                length = end - s
                if min_len <= length <= max_len and length >= max(a, b):
                    fwd_cost, rev_cost = (left_cost, right_cost) if strand == 0 else (right_cost, left_cost)
                    rows.append((s, end, i, strand, fwd_cost, rev_cost, 0))
    return rows


def expected(profile, pairs, text, k, min_len, max_len, rc, max_n_frac=None):
    """Searcher.hamming_amplicons(pairs, text, k, min_len, max_len) as a structured array, order (pair_idx, strand, start, end)."""
    rows = []
    for i, (fwd, rev) in enumerate(pairs):
        hits = href.expected(profile, [bytes(fwd), bytes(rev)], text, k, rc=True, max_n_frac=max_n_frac, without_trace=True)
        rows.extend(join(hits, i, len(fwd), len(rev), min_len, max_len, rc))
    return np.array(rows, dtype=DTYPE) if rows else np.zeros(0, dtype=DTYPE)


def same(got, want):
    """Field for field and in order."""
    return len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in FIELDS)


# The hand case: A x 150 + T x 150, F = R = AAAA, k = 0, 4 <= L <= 80.  '+' records: left starts 0 .. 146 (AAAA), right starts
# 150 .. 296 (TTTT = reverse_complement(AAAA)), d = p - s in [4, 76], d - 3 (s, p) each: sum = 73 * 74 / 2 = 2701.
HAND_TEXT = b"A" * 150 + b"T" * 150
HAND_PAIR = (b"AAAA", b"AAAA")
HAND_COUNT = 73 * 74 // 2
HAND_FIRST = (74, 154)   # the first left start with a partner: 150 - 76, and the first TTTT
HAND_LAST = (146, 226)   # the last AAAA with the farthest TTTT that max_len allows: 146 + 76 + 4
