"""The Hamming search restated in numpy, tied to the oracle: the profile relation comes out of the oracle's own DP (a one-row
pattern against all 256 byte values), H(s) = #{ j : !match(P[j], T[s + j]) } is a sum over numpy rows, and the expected
records -- both strands, the pattern-direction cigar, the float32 N rule -- are built from that.

ascii_ci is the Ascii relation on folded bytes (A-Z onto a-z), as the oracle has no profile of its own for it.
"""
import functools

import numpy as np

import oracle

_FOLD = np.arange(256, dtype=np.uint8)
_FOLD[65:91] += 32
_ALL = bytes(range(256))


@functools.lru_cache(maxsize=None)
def relation_row(profile: str, p: int) -> np.ndarray:
    """(256,) bool: row[t] = pattern byte p matches text byte t, read off the oracle's last DP row of the one-row pattern
    [p] over the text 0, 1, ..., 255 (cost 0 at column t + 1 iff byte t matches)."""
    if profile == "ascii_ci":
        return relation_row("ascii", int(_FOLD[p]))[_FOLD]
    row = oracle.last_row(profile, bytes([p]), _ALL)
    return row[1:] == 0


def mismatches(profile: str, pattern: bytes, text: bytes) -> np.ndarray:
    """H(s) for s = 0 .. n - m as int32 (empty if n < m)."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    m, n = len(pattern), len(t)
    if n < m:
        return np.zeros(0, dtype=np.int32)
    h = np.zeros(n - m + 1, dtype=np.int32)
    for j, p in enumerate(pattern):
        h += ~relation_row(profile, p)[t[j:j + n - m + 1]]
    return h


def _cigar(eq: np.ndarray) -> str:
    return oracle.rle_cigar(bytes(np.where(eq, ord("="), ord("X")).astype(np.uint8)))


def n_ok(count: int, m: int, max_n_frac) -> bool:
    """The reference's traced-span rule in float32."""
    return max_n_frac is None or bool(np.float32(count) / np.float32(m) <= np.float32(max_n_frac))


def expected(profile: str, patterns, text: bytes, k: int, rc: bool = False, max_n_frac=None, without_trace: bool = False):
    """The records of Searcher.search_hamming as oracle.Match objects, in the contract's order: pattern_idx, '+' before
    '-', text_start.  max_n_frac = 1.0 is no filter, as everywhere."""
    if isinstance(patterns, (bytes, bytearray)):
        patterns = [patterns]
    if max_n_frac is not None and max_n_frac == 1.0:
        max_n_frac = None
    text = bytes(text)
    t = np.frombuffer(text, dtype=np.uint8)
    is_n = np.concatenate(([0], np.cumsum((t | 0x20) == 0x6E))).astype(np.int64)
    out = []
    for idx, pat in enumerate(patterns):
        pat = bytes(pat)
        m = len(pat)
        for strand in ("+", "-") if rc else ("+",):
            scanned = pat if strand == "+" else oracle.reverse_complement(profile, pat)
            h = mismatches(profile, scanned, text)
            starts = [s for s in np.nonzero(h <= k)[0].tolist() if n_ok(int(is_n[s + m] - is_n[s]), m, max_n_frac)]
            if starts and not without_trace:
                rel = np.stack([relation_row(profile, c) for c in scanned])  # (m, 256)
                cols = np.arange(m)
                eq_all = rel[cols[None, :], t[np.asarray(starts)[:, None] + cols[None, :]]]  # (hits, m)
            for i, s in enumerate(starts):
                cigar = ""
                if not without_trace:
                    cigar = _cigar(eq_all[i] if strand == "+" else eq_all[i][::-1])  # '-': in pattern direction
                out.append(oracle.Match(idx, s, s + m, 0, m, int(h[s]), strand, cigar))
    return out


def expected_table(profile: str, patterns, text: bytes, k: int, rc: bool = False, max_n_frac=None):
    """The same hits as four numpy columns (pattern_idx, strand 0 / 1, text_start, cost) in the contract's order: for
    results too large to compare as Python objects."""
    if isinstance(patterns, (bytes, bytearray)):
        patterns = [patterns]
    if max_n_frac is not None and max_n_frac == 1.0:
        max_n_frac = None
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    is_n = np.concatenate(([0], np.cumsum((t | 0x20) == 0x6E))).astype(np.int64)
    cols = [[], [], [], []]
    for idx, pat in enumerate(patterns):
        pat = bytes(pat)
        m = len(pat)
        for strand in (0, 1) if rc else (0,):
            h = mismatches(profile, pat if strand == 0 else oracle.reverse_complement(profile, pat), text)
            keep = h <= k
            if max_n_frac is not None and len(h):
                cnt = is_n[m:m + len(h)] - is_n[:len(h)]
                keep &= (cnt.astype(np.float32) / np.float32(m)) <= np.float32(max_n_frac)
            s = np.nonzero(keep)[0]
            for c, v in zip(cols, (np.full(len(s), idx), np.full(len(s), strand), s, h[s])):
                c.append(v.astype(np.int64))
    return tuple(np.concatenate(c) if c else np.zeros(0, dtype=np.int64) for c in cols)


def key(m):
    return (m.pattern_idx, m.text_start, m.text_end, m.pattern_start, m.pattern_end, m.cost, m.strand, m.cigar)
