"""Searcher.hamming_pairs / hamming_nearest restated in numpy: a brute force over all (i, j), built from hamming_ref's
relation (read off the oracle's DP) and the oracle's reverse complement -- no second copy of either.

H(x, y) = #{ t : !match(x[t], y[t]) }; strand 1 is H(x, reverse_complement(y)).  Two-set mode: every (i, j, strand) with cost
<= k.  Self mode (b is None): strand 0 for i < j, strand 1 for i <= j.  Nearest: of all (j, strand) with cost <= k -- in self
mode the full square without (i, i, 0) -- the smallest under (cost, j, strand), and how many share its cost.
"""
import numpy as np

import oracle

import hamming_ref as href

PAIR = np.dtype([("a_idx", "<u4"), ("b_idx", "<u4"), ("cost", "u1"), ("strand", "u1")])
NO_MATCH = 255


def _rows(seqs) -> np.ndarray:
    if isinstance(seqs, np.ndarray):
        return seqs
    seqs = [bytes(s) for s in seqs]
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), len(seqs[0]) if seqs else 0)


def relation(profile: str) -> np.ndarray:
    """(256, 256) bool: [p, t] = byte p matches byte t."""
    return np.stack([href.relation_row(profile, p) for p in range(256)])


def distances(profile: str, a, b, rc: bool) -> np.ndarray:
    """(n_a, n_b, S) int32, S = 2 for rc: H(a_i, b_j) and H(a_i, reverse_complement(b_j))."""
    a, b = _rows(a), _rows(b)
    rel = relation(profile)
    targets = [b]
    if rc:
        targets.append(_rows([oracle.reverse_complement(profile, bytes(row)) for row in b]) if len(b) else b)
    out = np.zeros((len(a), len(b), len(targets)), dtype=np.int32)
    for s, tb in enumerate(targets):
        for t in range(a.shape[1]):
            out[:, :, s] += ~rel[a[:, t][:, None], tb[:, t][None, :]]
    return out


def _records(h, k, rc, self_mode, square):
    keep = h <= k
    if self_mode:
        i = np.arange(h.shape[0])[:, None]
        j = np.arange(h.shape[1])[None, :]
        if square:
            keep[:, :, 0] &= i != j
        else:
            keep[:, :, 0] &= j > i
            if rc:
                keep[:, :, 1] &= j >= i
    i, j, s = np.nonzero(keep)  # (row-major: ascending (i, j, strand))
    out = np.zeros(len(i), dtype=PAIR)
    out["a_idx"], out["b_idx"], out["strand"], out["cost"] = i, j, s, h[i, j, s]
    return out


def expected_pairs(profile: str, a, b, k: int, rc: bool = False, square: bool = False) -> np.ndarray:
    """The records in the contract's order (a_idx, b_idx, strand).  square: self mode as hamming_nearest sees it."""
    self_mode = b is None
    return _records(distances(profile, a, a if self_mode else b, rc), k, rc, self_mode, square)


def expected_self(profile: str, a, k: int, rc: bool = False):
    """(expected_pairs(a, None), expected_pairs(a, None, square=True)) from one table of distances."""
    h = distances(profile, a, a, rc)
    return _records(h, k, rc, True, False), _records(h, k, rc, True, True)


def nearest_of_pairs(pairs: np.ndarray, n_a: int):
    """(cost, index, strand, ties) from records in contract order: per a_idx the first record of the smallest cost."""
    cost = np.full(n_a, NO_MATCH, dtype=np.uint8)
    index = np.full(n_a, 0xFFFFFFFF, dtype=np.uint32)
    strand = np.zeros(n_a, dtype=np.uint8)
    ties = np.zeros(n_a, dtype=np.uint32)
    for r in pairs:
        i = int(r["a_idx"])
        if r["cost"] < cost[i]:
            cost[i], index[i], strand[i], ties[i] = r["cost"], r["b_idx"], r["strand"], 1
        elif r["cost"] == cost[i]:
            ties[i] += 1
    return cost, index, strand, ties


def expected_nearest(profile: str, a, b, k: int, rc: bool = False):
    return nearest_of_pairs(expected_pairs(profile, a, b, k, rc, square=True), len(_rows(a)))


def as_tuples(records) -> list:
    return [(int(r["a_idx"]), int(r["b_idx"]), int(r["strand"]), int(r["cost"])) for r in records]


# ---- a case written out by hand (dna) ----
# reverse complements: ACGT -> ACGT, ACGA -> TCGT, TTTT -> AAAA, AAAT -> ATTT
HAND_SELF = [b"ACGT", b"ACGA", b"TTTT", b"AAAT"]
HAND_K = 1
# (a_idx, b_idx, strand, cost): ACGT is its own reverse complement; ACGT / ACGA differ in the last base, on either strand;
# TTTT against reverse_complement(AAAT) = ATTT differs in the first
HAND_SELF_PAIRS_RC = [(0, 0, 1, 0), (0, 1, 0, 1), (0, 1, 1, 1), (2, 3, 1, 1)]
HAND_SELF_PAIRS_FWD = [(0, 1, 0, 1)]
# per entry (cost, index, strand, ties): the square without (i, i, 0)
HAND_SELF_NEAREST_RC = [(0, 0, 1, 1), (1, 0, 0, 2), (1, 3, 1, 1), (1, 2, 1, 1)]
HAND_SELF_NEAREST_FWD = [(1, 1, 0, 1), (1, 0, 0, 1), (NO_MATCH, 0xFFFFFFFF, 0, 0), (NO_MATCH, 0xFFFFFFFF, 0, 0)]
HAND_A = [b"ACGT", b"GGGG"]
HAND_B = [b"ACGA", b"ACGT", b"CCCC"]
HAND_TWO_PAIRS = [(0, 0, 0, 1), (0, 1, 0, 0)]
HAND_TWO_NEAREST = [(0, 1, 0, 1), (NO_MATCH, 0xFFFFFFFF, 0, 0)]
