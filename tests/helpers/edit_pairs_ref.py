"""Searcher.edit_pairs / edit_nearest restated in numpy: the full DP of every (i, j) at once, built from hamming_ref's relation
(read off the oracle's DP) and the oracle's reverse complement; records and nearest through hamming_pairs_ref's own
`_records` / `nearest_of_pairs` on the table of distances -- no second copy of the contract's order, triangle or tie rule.

E(x, y) = D[m_a][m_b], D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + !match(x[i-1], y[j-1]), D[i-1][j] + 1,
D[i][j-1] + 1); strand 1 is E(x, reverse_complement(y)).  No bit vectors here: a column of D is computed from the one before
it as t[i] = min(D[i-1][j-1] + sub, D[i][j-1] + 1) and then D[i][j] = min(t[i], D[i-1][j] + 1), which unrolls to
D[i][j] = i + min_{i' <= i} (t[i'] - i') -- a running minimum along the rows.
"""
import numpy as np

import oracle

import hamming_pairs_ref as pref

NO_MATCH = pref.NO_MATCH
as_tuples = pref.as_tuples
nearest_of_pairs = pref.nearest_of_pairs


def edit_table(rel: np.ndarray, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """(n_a, n_b) int32: E(a_i, b_j) for sequences of m_a and m_b bytes under the relation rel[p, t]."""
    n_a, m_a = a.shape
    n_b, m_b = b.shape
    assert m_a <= 64 and m_b <= 64  # (int8 holds every value below: D <= 64, D + 1 <= 65, t[i] - i >= -64)
    out = np.zeros((n_a, n_b), dtype=np.int32)
    rows = np.arange(m_a + 1, dtype=np.int8)
    block = max(1, (1 << 23) // max(1, n_b * (m_a + 1)))  # entries of a per turn: the columns stay within a few MiB
    for i0 in range(0, n_a, block):
        ab = a[i0:i0 + block]
        miss = (~rel[ab[None, :, :], np.arange(256)[:, None, None]]).astype(np.int8)  # [c, i, t] = !match(a_i[t], c)
        col = np.broadcast_to(rows, (n_b, len(ab), m_a + 1)).copy()  # [j, i, .]: D[.][0] = i
        for j in range(m_b):
            sub = miss[b[:, j]]  # (n_b, block, m_a): !match(x[i-1], y[j])
            t = np.empty_like(col)
            t[:, :, 0] = j + 1
            np.minimum(col[:, :, :-1] + sub, col[:, :, 1:] + 1, out=t[:, :, 1:])
            t -= rows
            np.minimum.accumulate(t, axis=2, out=t)
            t += rows
            col = t
        out[i0:i0 + block] = col[:, :, m_a].T
    return out


def distances(profile: str, a, b, rc: bool) -> np.ndarray:
    """(n_a, n_b, S) int32, S = 2 for rc: E(a_i, b_j) and E(a_i, reverse_complement(b_j))."""
    a, b = pref._rows(a), pref._rows(b)
    rel = pref.relation(profile)
    targets = [b]
    if rc:
        targets.append(pref._rows([oracle.reverse_complement(profile, bytes(row)) for row in b]) if len(b) else b)
    return np.stack([edit_table(rel, a, tb) for tb in targets], axis=2)


def plain_distance(profile: str, x: bytes, y: bytes) -> int:
    """E(x, y) cell by cell, as the definition reads: what edit_table is checked against."""
    rel = pref.relation(profile)
    d = [[0] * (len(y) + 1) for _ in range(len(x) + 1)]
    for i in range(len(x) + 1):
        d[i][0] = i
    for j in range(len(y) + 1):
        d[0][j] = j
    for i in range(1, len(x) + 1):
        for j in range(1, len(y) + 1):
            d[i][j] = min(d[i - 1][j - 1] + (0 if rel[x[i - 1], y[j - 1]] else 1), d[i - 1][j] + 1, d[i][j - 1] + 1)
    return d[len(x)][len(y)]


def expected_pairs(profile: str, a, b, k: int, rc: bool = False, square: bool = False) -> np.ndarray:
    """The records in the contract's order (a_idx, b_idx, strand).  square: self mode as edit_nearest sees it."""
    self_mode = b is None
    return pref._records(distances(profile, a, a if self_mode else b, rc), k, rc, self_mode, square)


def expected_self(profile: str, a, k: int, rc: bool = False):
    """(expected_pairs(a, None), expected_pairs(a, None, square=True)) from one table of distances."""
    e = distances(profile, a, a, rc)
    return pref._records(e, k, rc, True, False), pref._records(e, k, rc, True, True)


def expected_nearest(profile: str, a, b, k: int, rc: bool = False):
    return nearest_of_pairs(expected_pairs(profile, a, b, k, rc, square=True), len(pref._rows(a)))


# ---- a case written out by hand (dna, forward, k = 2) ----
# CGTA is ACGT with its first base moved to the end: one deletion and one insertion, and Hamming distance 4; ACTG swaps the
# last two bases: two substitutions; TTTT keeps only the last base: 3
HAND_A = [b"ACGT"]
HAND_B = [b"CGTA", b"ACGT", b"TTTT", b"ACTG"]
HAND_K = 2
HAND_PAIRS = [(0, 0, 0, 2), (0, 1, 0, 0), (0, 3, 0, 2)]  # (a_idx, b_idx, strand, cost)
HAND_NEAREST = [(0, 1, 0, 1)]                            # (cost, index, strand, ties)


# ---- inputs with indels in them ----
def mutate(rng, seq: np.ndarray, edits: int, m_out: int, alphabet: np.ndarray) -> np.ndarray:
    """`seq` after `edits` random substitutions, insertions and deletions, padded with random letters or cut to m_out."""
    s = list(seq)
    for _ in range(edits):
        op = rng.integers(3)
        if op == 0 and s:
            s[rng.integers(len(s))] = alphabet[rng.integers(len(alphabet))]
        elif op == 1:
            s.insert(rng.integers(len(s) + 1), alphabet[rng.integers(len(alphabet))])
        elif s:
            del s[rng.integers(len(s))]
    while len(s) < m_out:
        s.append(alphabet[rng.integers(len(alphabet))])
    return np.array(s[:m_out], dtype=np.uint8)


ALPHABETS = {"dna": b"ACGT", "iupac": b"ACGTACGTACGTNRYKM", "ascii": b"abcdefgh", "ascii_ci": b"abcdABCD"}


def related_lists(profile: str, n_a: int, n_b: int, m_a: int, m_b: int, k: int, seed: int):
    """(a, b): a random, 20 % of it an earlier entry of a with 0 .. k random edits (self mode has something to find); 70 % of
    b an entry of a with 0 .. k random edits, padded or cut to m_b, the rest random."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(ALPHABETS[profile], dtype=np.uint8)
    a = alphabet[rng.integers(len(alphabet), size=(n_a, m_a))]
    b = alphabet[rng.integers(len(alphabet), size=(n_b, m_b))]
    for i in range(1, n_a):
        if rng.random() < 0.2:
            a[i] = mutate(rng, a[rng.integers(i)], int(rng.integers(k + 1)), m_a, alphabet)
    for j in range(n_b):
        if rng.random() < 0.7:
            b[j] = mutate(rng, a[rng.integers(n_a)], int(rng.integers(k + 1)), m_b, alphabet)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)
