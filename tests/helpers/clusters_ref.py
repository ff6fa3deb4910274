"""Searcher.hamming_clusters / edit_clusters restated: the edges are the self-mode records of hamming_pairs_ref /
edit_pairs_ref (brute force over all (i, j)) with (i, i, 1) dropped, the components a plain union-find over them.

labels[i] = the smallest index of i's connected component, sizes[i] = the size of that component.
"""
import numpy as np

import edit_pairs_ref as eref
import hamming_pairs_ref as pref


def components(n: int, edges):
    """(labels, sizes), uint32, of the graph on 0 .. n - 1 with the given (i, j) edges."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in edges:
        ri, rj = find(int(i)), find(int(j))
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)  # (the smaller index stays the root: a root is its tree's minimum)
    labels = np.array([find(x) for x in range(n)], dtype=np.uint32)
    sizes = np.bincount(labels, minlength=n)[labels].astype(np.uint32)
    return labels, sizes


def components_fast(n: int, i, j):
    """components()'s labels for index arrays i, j without a Python loop over the edges: every node takes the smallest label
    at the other end of its edges, then the label of its label, until nothing moves (as many turns as a component is wide)."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    lab = np.arange(n, dtype=np.int64)
    while True:
        low = np.minimum(lab[i], lab[j])
        new = lab.copy()
        np.minimum.at(new, i, low)
        np.minimum.at(new, j, low)
        new = new[new]
        if np.array_equal(new, lab):
            return lab.astype(np.uint32)
        lab = new


def edges_of_records(records):
    """The (i, j) of pair records without the self edges (i, i, 1)."""
    keep = records["a_idx"] != records["b_idx"]
    return zip(records["a_idx"][keep].tolist(), records["b_idx"][keep].tolist())


def expected_clusters(profile: str, a, k: int, rc: bool = False, edit: bool = False):
    ref = eref if edit else pref
    a = pref._rows(a)
    return components(len(a), edges_of_records(ref.expected_pairs(profile, a, None, k, rc=rc)))


# ---- a case written out by hand (dna, k = 1) ----
# forward: ACGT - ACGA (last base) - ACCA (third base) is a chain, ACGT / ACCA are two apart; TTTT and AAAT are alone.
# rc: reverse_complement(AAAT) = ATTT is one from TTTT, which joins 3 and 4; ACGT is its own reverse complement -- (0, 0, 1)
# is a record of the pair call and no edge
HAND = [b"ACGT", b"ACGA", b"ACCA", b"TTTT", b"AAAT"]
HAND_K = 1
HAND_FWD = ([0, 0, 0, 3, 4], [3, 3, 3, 1, 1])   # (labels, sizes)
HAND_RC = ([0, 0, 0, 3, 3], [3, 3, 3, 2, 2])
