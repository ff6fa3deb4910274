"""Searcher.umi_groups restated: duplicates by a Python dict on the folded sequence, neighbours from hamming_pairs_ref's brute
force on the distinct sequences, `cluster` through clusters_ref's union-find, `directional` as the SEQUENTIAL procedure of
UMI-tools -- sort by (count descending, first index ascending), open a group at the first sequence that has none, take what a
breadth-first search along the count-rule edges reaches and that has none yet.  It is deliberately not the
minimum-over-ancestors form the device computes: comparing the two checks that equivalence.

(labels, sizes, reps, counts), uint32, n entries: reps[i] the first index with i's folded sequence, counts[i] how many share
it, labels[i] the first index of the opener of i's group, sizes[i] the READS with that label.
"""
from collections import deque

import numpy as np

import clusters_ref as cref
import hamming_pairs_ref as pref

METHODS = ("unique", "cluster", "directional")


def fold_table(profile: str) -> np.ndarray:
    """(256,) uint8: per byte the smallest byte that matches exactly the same bytes -- two sequences are duplicates when they
    fold to the same bytes (dna: the 2-bit code, so case and everything that shares a code; iupac: the letter's set of bases,
    so case and T / U, while N and A stay apart; ascii: nothing; ascii_ci: A-Z onto a-z)."""
    rel = pref.relation(profile)
    first = {}
    return np.array([first.setdefault(rel[c].tobytes(), c) for c in range(256)], dtype=np.uint8)


def duplicates(profile: str, a):
    """(reps, counts) of the rows of a."""
    rows = fold_table(profile)[pref._rows(a)]
    first, reps = {}, []
    for i, row in enumerate(rows):
        reps.append(first.setdefault(row.tobytes(), i))
    reps = np.array(reps, dtype=np.uint32)
    counts = np.bincount(reps, minlength=len(reps))[reps].astype(np.uint32)
    return reps, counts


def directional_groups(counts, neighbours):
    """The opener of every distinct sequence's group, UMI-tools' way.  counts[u]; neighbours: (u, v) pairs, u != v."""
    n_u = len(counts)
    out = [[] for _ in range(n_u)]
    for u, v in neighbours:
        if counts[u] >= 2 * counts[v] - 1:
            out[u].append(v)
        if counts[v] >= 2 * counts[u] - 1:
            out[v].append(u)
    opener = [-1] * n_u
    for u in sorted(range(n_u), key=lambda x: (-int(counts[x]), x)):
        if opener[u] >= 0:
            continue
        opener[u] = u
        queue = deque([u])
        while queue:
            x = queue.popleft()
            for y in out[x]:
                if opener[y] < 0:  # (one that has a group was reached by an earlier opener, and so was all behind it)
                    opener[y] = u
                    queue.append(y)
    return opener


def expected_umi_groups(profile: str, a, k: int, method: str = "directional", rc: bool = False):
    assert method in METHODS
    a = pref._rows(a)
    n, m = a.shape
    reps, counts = duplicates(profile, a)
    first = np.flatnonzero(reps == np.arange(n))              # the distinct sequences, ascending first index
    if method == "unique":
        group = np.arange(len(first))
    else:
        records = pref.expected_pairs(profile, a[first], None, min(k, m), rc=rc)
        edges = list(cref.edges_of_records(records))        # ((u, u, 1) dropped)
        if method == "cluster":
            group = cref.components(len(first), edges)[0]
        else:
            group = np.array(directional_groups(counts[first], edges), dtype=np.int64)
    dense = np.cumsum(reps == np.arange(n)) - 1               # dense[i] for i = first[u] is u
    labels = first[group[dense[reps]]].astype(np.uint32)
    sizes = np.bincount(labels, minlength=n)[labels].astype(np.uint32)
    return labels, sizes, reps, counts


# ---- a case written out by hand (dna, k = 1, no rc): AAAA x 10, AAAT x 4, AATT x 3 and one CCCC, interleaved ----
# AAAA -> AAAT holds (10 >= 2 * 4 - 1 = 7); AAAT -> AATT does not (4 < 2 * 3 - 1 = 5), nor AATT -> AAAT (3 < 7); AAAA and AATT
# are two apart.  directional: {AAAA, AAAT}, {AATT}, {CCCC}; cluster joins the first three; unique keeps four.
HAND = [b"AAAA", b"AAAT", b"AATT", b"AAAA", b"CCCC", b"AAAA", b"AAAT", b"AAAA", b"AATT", b"AAAA", b"AAAT", b"AAAA", b"AAAA", b"AATT",
        b"AAAT", b"AAAA", b"AAAA", b"AAAA"]
HAND_K = 1
HAND_REPS = [0, 1, 2, 0, 4, 0, 1, 0, 2, 0, 1, 0, 0, 2, 1, 0, 0, 0]
HAND_COUNTS = [10, 4, 3, 10, 1, 10, 4, 10, 3, 10, 4, 10, 10, 3, 4, 10, 10, 10]
HAND_LABELS = {"unique": HAND_REPS,
               "cluster": [0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
               "directional": [0, 0, 2, 0, 4, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, 0, 0, 0]}
HAND_SIZES = {"unique": HAND_COUNTS,
              "cluster": [17, 17, 17, 17, 1, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17],
              "directional": [14, 14, 3, 14, 1, 14, 14, 14, 3, 14, 14, 14, 14, 3, 14, 14, 14, 14]}
