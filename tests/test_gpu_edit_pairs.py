"""Searcher.edit_pairs / edit_nearest on the device against tests/helpers/edit_pairs_ref.py (the full DP in numpy, built from
the oracle's relation and reverse complement): records compared for exact equality, array to array, order included.  The
sizes are the smallest at which the kernels can go wrong -- every instantiation (planes x words), lengths on both sides of
the word border, the seams of the staged tiles, of a wavefront, of a strip and of a chunk, the diagonal of self mode -- not a
workload.  Every case's inputs hold pairs that only an insertion or deletion brings within k, so neither an empty nor a
Hamming-only answer passes."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import oracle  # noqa: E402
import edit_pairs_ref as eref  # noqa: E402
import hamming_pairs_ref as pref  # noqa: E402

pytestmark = pytest.mark.gpu

ALPHABETS = (("dna", False), ("dna", True), ("iupac", False), ("iupac", True), ("ascii", False), ("ascii_ci", False))
SHAPES = ((16, 16, 2), (32, 33, 3), (33, 31, 2), (64, 64, 4), (5, 7, 2), (1, 1, 0), (64, 1, 63))  # (m_a, m_b, k)
PLANES = {"dna": 2, "iupac": 4, "ascii": 8, "ascii_ci": 8}
TILE_WORDS = 2048  # edit_pairs.hip: kEditTileWords


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


def fields(records):
    return [records[f].tolist() for f in ("a_idx", "b_idx", "strand", "cost")]


def check_pairs(got, want):
    assert len(got) == len(want), (len(got), len(want))
    assert fields(got) == fields(want)
    assert not got["pad_"].any()


def check_nearest(got, want):
    for g, w, name in zip(got, want, ("cost", "index", "strand", "ties")):
        assert g.dtype == w.dtype and g.tolist() == w.tolist(), name


def records_per_tile(profile, m_b):
    """edit_pairs.hip: a record is one row code per column, 32 / P columns to a word; a staged tile holds 2048 words"""
    return TILE_WORDS // -(-m_b * PLANES[profile] // 32)


# ---------------------------------------------------------------- (1) profiles and lengths
@functools.lru_cache(maxsize=None)
def shape_case(alphabet, shape):
    profile, rc = ALPHABETS[alphabet]
    m_a, m_b, k = SHAPES[shape]
    n_a, n_b = (150, 170) if max(m_a, m_b) >= 32 else (300, 260)
    a, b = eref.related_lists(profile, n_a, n_b, m_a, m_b, k, seed=100 * alphabet + shape)
    two = eref.distances(profile, a, b, rc)
    own = eref.distances(profile, a, a, rc)
    return profile, rc, m_a, m_b, k, a, b, two, own


@pytest.mark.parametrize("shape", range(len(SHAPES)))
@pytest.mark.parametrize("alphabet", range(len(ALPHABETS)))
def test_profiles_and_lengths(sassy, alphabet, shape):
    """Every profile and strand setting at every (m_a, m_b, k) of the list, both calls, two-set and self mode (self mode
    compares a with itself: m_b = m_a).  70 % of b is an entry of a after 0 .. k random substitutions, insertions and
    deletions.  Where the lengths are equal and k >= 2 at least 20 expected records have E <= k < H and every cost 0 .. k
    turns up; an equal-length pair with E <= k < H needs an insertion and a deletion, so (1, 1, 0) cannot hold one: there
    E = H and the case asserts its records and both costs' presence only.  Unequal lengths: at least 20 records."""
    profile, rc, m_a, m_b, k, a, b, two, own = shape_case(alphabet, shape)
    want = pref._records(two, k, rc, False, False)
    if m_a == m_b:
        hamming = pref.distances(profile, a, b, rc)
        beyond = int(((two <= k) & (hamming > k)).sum())
        print(f"{profile} rc={rc} ({m_a}, {m_b}, {k}): records={len(want)} with E <= k < H: {beyond} costs={sorted(set(want['cost'].tolist()))}")
        assert sorted(set(want["cost"].tolist())) == list(range(k + 1))
        assert beyond >= 20 or k < 2
    assert len(want) >= 20
    s = sassy.Searcher(profile, rc=rc)
    check_pairs(s.edit_pairs(a, b, k), want)
    assert s.stats()["filtered"] == 9 and s.stats()["candidates"] == len(want)
    check_nearest(s.edit_nearest(a, b, k), pref.nearest_of_pairs(want, len(a)))
    # self mode: the triangle for the records, the square without (i, i, 0) for nearest
    check_pairs(s.edit_pairs(a, None, k), pref._records(own, k, rc, True, False))
    check_nearest(s.edit_nearest(a, None, k), pref.nearest_of_pairs(pref._records(own, k, rc, True, True), len(a)))


def test_hand_written_case(sassy):
    s = sassy.Searcher("dna", rc=False)
    assert eref.as_tuples(s.edit_pairs(eref.HAND_A, eref.HAND_B, eref.HAND_K)) == eref.HAND_PAIRS
    cost, index, strand, ties = s.edit_nearest(eref.HAND_A, eref.HAND_B, eref.HAND_K)
    assert [(int(cost[0]), int(index[0]), int(strand[0]), int(ties[0]))] == eref.HAND_NEAREST


# ---------------------------------------------------------------- (2) extremes of k
@pytest.mark.parametrize("alphabet", range(len(ALPHABETS)))
def test_extremes_of_k(sassy, alphabet):
    """k = 0; k >= max(m_a, m_b), where every visited pair is a record (254 too: k is cut to the longer length); and lengths
    further apart than k: an empty answer and, by the stats, no launch."""
    profile, rc = ALPHABETS[alphabet]
    S = 2 if rc else 1
    a, b = eref.related_lists(profile, 130, 90, 9, 7, 2, seed=alphabet)
    b[::3] = a[:30, :7]  # (prefixes: E = 2)
    two, own = eref.distances(profile, a, b, rc), eref.distances(profile, a, a, rc)
    s = sassy.Searcher(profile, rc=rc)
    for k in (0, 2, 9, 254):
        want = pref._records(two, k, rc, False, False)
        check_pairs(s.edit_pairs(a, b, k), want)
        check_nearest(s.edit_nearest(a, b, k), pref.nearest_of_pairs(want, len(a)))
        check_pairs(s.edit_pairs(a, None, k), pref._records(own, k, rc, True, False))
        check_nearest(s.edit_nearest(a, None, k), pref.nearest_of_pairs(pref._records(own, k, rc, True, True), len(a)))
        if k >= 9:
            assert len(want) == 130 * 90 * S
    equal = a[:, :7].copy()  # (k = 0 with something to find)
    check_pairs(s.edit_pairs(equal, b, 0), pref._records(eref.distances(profile, equal, b, rc), 0, rc, False, False))
    assert s.stats()["candidates"] >= 30
    for k in (0, 1):  # |m_a - m_b| = 2 > k
        assert len(s.edit_pairs(a, b, k)) == 0
        st = s.stats()
        assert st["filtered"] == 9 and st["scan_launches"] == 0 and st["candidates"] == 0
        cost, index, strand, ties = s.edit_nearest(a, b, k)
        assert s.stats()["scan_launches"] == 0
        assert (cost == eref.NO_MATCH).all() and (index == 0xFFFFFFFF).all() and not strand.any() and not ties.any()
        assert len(cost) == len(index) == len(strand) == len(ties) == len(a)


# ---------------------------------------------------------------- (3) the seams of the staged tiles
# (profile, rc, m): one case per instantiation planes x words.  m_a = m_b = m, so that self mode runs the same instantiation.
# A remainder that is no multiple of U needs U > S (records come S to a target): the one-word cases (U = 4) take rc, the
# two-word cases (U = 2) do not.
SEAM_CASES = (("dna", True, 32), ("dna", False, 33), ("iupac", True, 32), ("iupac", False, 64), ("ascii", False, 32), ("ascii_ci", False, 64))
SEAM_K = 2
CHUNKS = (1, 3, 7)


def seam_targets(S, seam):
    """the two targets whose records end before the seam, the two whose records begin at it (T is even in every case)"""
    return ((seam - 1) // S - 1, (seam - 1) // S), (seam // S, seam // S + 1)


def planted_targets(profile, rc, m, n_b):
    """targets on both sides of the first two tile seams of a walk that starts at record 0, and the last ones of the list"""
    S, T = (2 if rc else 1), records_per_tile(profile, m)
    at = {n_b - 3, n_b - 2, n_b - 1}
    for seam in (T, 2 * T):
        before, after = seam_targets(S, seam)
        at |= set(before) | set(after)
    return sorted(j for j in at if 0 <= j < n_b)


def within_two_edits(rng, seq, q, m, alphabet):
    """one random edit -- padded or cut back to m that is at most two -- or a shift by one row: a deletion and an insertion"""
    return np.roll(seq, 1) if q % 3 == 0 else eref.mutate(rng, seq, 1, m, alphabet)


@functools.lru_cache(maxsize=None)
def seam_case(t):
    profile, rc, m = SEAM_CASES[t]
    S, T = (2 if rc else 1), records_per_tile(profile, m)
    n_b = (2 * T + 8 - S) // S  # two full tiles and a third of 7 (S = 1) or 6 (S = 2) records: rounds of U, then a rest
    rng = np.random.default_rng(70 + t)
    alphabet = np.frombuffer(eref.ALPHABETS[profile], dtype=np.uint8)
    a = alphabet[rng.integers(len(alphabet), size=(70, m))]  # two wavefronts, the second with 6 entries
    b = alphabet[rng.integers(len(alphabet), size=(n_b, m))]
    plants = planted_targets(profile, rc, m, n_b)
    for q, j in enumerate(plants):
        near = within_two_edits(rng, a[(7 * q) % 70], q, m, alphabet)
        b[j] = np.frombuffer(oracle.reverse_complement(profile, near.tobytes()), dtype=np.uint8) if rc and q % 2 else near
    return profile, rc, m, a, b, plants, eref.distances(profile, a, b, rc)


@pytest.mark.parametrize("t", range(len(SEAM_CASES)))
def test_staged_tile_seams_two_sets(sassy, t):
    """Per instantiation more than two staged tiles of target records and a third that no round of U records divides;
    records planted on both sides of both seams (with rc a seam may part a target's two strands); chunk counts 1, 3 and 7
    move the seams and must not move the answer."""
    profile, rc, m, a, b, plants, table = seam_case(t)
    S, T = (2 if rc else 1), records_per_tile(profile, m)
    U = 4 if m <= 32 else 2  # (edit_pairs.hip: edit_unroll)
    assert T % 2 == 0 and 0 < len(b) * S - 2 * T < T and (len(b) * S - 2 * T) % U != 0
    want = pref._records(table, SEAM_K, rc, False, False)
    hit = set(want["b_idx"].tolist())
    print(f"{profile} rc={rc} m={m}: T={T} n_b={len(b)} records={len(want)} planted={plants} found={sorted(hit & set(plants))}")
    assert set(plants) <= hit
    for seam in (T, 2 * T):  # records on either side of each seam
        before, after = seam_targets(S, seam)
        assert set(before) <= hit and set(after) <= hit and before[1] * S + S - 1 == seam - 1 and after[0] * S == seam
    s = sassy.Searcher(profile, rc=rc)
    for chunks in CHUNKS:
        s.set_option("pairs_chunks", chunks)
        check_pairs(s.edit_pairs(a, b, SEAM_K), want)
        assert s.stats()["chunks"] == chunks
        check_nearest(s.edit_nearest(a, b, SEAM_K), pref.nearest_of_pairs(want, len(a)))


# self mode: the targets are the entries, and a strip's walk starts at its own first entry, wavefront w of it 64 w S records
# further on.  With tiles of T records that is at a seam, inside a tile or behind the first tile only where T <= 192 S, which
# the record sizes allow for Ascii at m = 64 (T = 128: wavefront 1 inside tile 0, 2 at the seam, 3 inside tile 1, behind tile
# 0) and Iupac with rc at m = 48 (T = 341, 128 w records: wavefronts 1 and 2 inside tile 0, 3 inside tile 1, behind tile 0).
# Dna's records are at most 4 words (T >= 512): every wavefront of a strip starts inside the strip's first tile; the Dna
# case (m = 17: T = 1024 records, 512 targets) has a seam in the walks of its first strip all the same.
SELF_SEAM_CASES = (("ascii", False, 64, 260), ("iupac", True, 48, 260), ("dna", True, 17, 530))


@functools.lru_cache(maxsize=None)
def self_seam_case(t):
    profile, rc, m, n = SELF_SEAM_CASES[t]
    S, T = (2 if rc else 1), records_per_tile(profile, m)
    rng = np.random.default_rng(170 + t)
    alphabet = np.frombuffer(eref.ALPHABETS[profile], dtype=np.uint8)
    a = alphabet[rng.integers(len(alphabet), size=(n, m))]
    # near copies of earlier entries on both sides of every wavefront's start and of the first two seams behind it
    at = set()
    for w in range(0, n, 64):
        for r in (w * S, w * S + T, w * S + 2 * T):
            at |= {(r - 1) // S, r // S, r // S + 1}
    at = sorted(j for j in at if 2 <= j < n)
    for q, j in enumerate(at):
        src = a[(j - 1 - 5 * (q % 7)) % j]
        near = within_two_edits(rng, src, q, m, alphabet)
        a[j] = np.frombuffer(oracle.reverse_complement(profile, near.tobytes()), dtype=np.uint8) if rc and q % 2 else near
    return profile, rc, m, np.ascontiguousarray(a), at, eref.distances(profile, a, a, rc)


@pytest.mark.parametrize("t", range(len(SELF_SEAM_CASES)))
def test_staged_tile_seams_self_mode(sassy, t):
    profile, rc, m, a, at, table = self_seam_case(t)
    want = pref._records(table, SEAM_K, rc, True, False)
    square = pref._records(table, SEAM_K, rc, True, True)
    hit = set(want["b_idx"].tolist())
    print(f"{profile} rc={rc} m={m}: T={records_per_tile(profile, m)} n={len(a)} records={len(want)} planted={len(at)} found={len(hit & set(at))}")
    assert set(at) <= hit
    s = sassy.Searcher(profile, rc=rc)
    for chunks in CHUNKS:
        s.set_option("pairs_chunks", chunks)
        check_pairs(s.edit_pairs(a, None, SEAM_K), want)
        check_nearest(s.edit_nearest(a, None, SEAM_K), pref.nearest_of_pairs(square, len(a)))


# ---------------------------------------------------------------- (4) the strip's edge, the triangle
@pytest.mark.parametrize("n_a", (255, 256, 257))
def test_strip_edge(sassy, n_a):
    """one strip short of an entry, exactly one, one entry into the second; the last entries are the ones with partners"""
    profile, rc, m_a, m_b, k = "dna", True, 16, 17, 2
    a, b = eref.related_lists(profile, n_a, 97, m_a, m_b, k, seed=n_a)
    for q, i in enumerate(range(250, n_a)):
        b[q] = np.insert(a[i], 2 * q, ord("A"))  # (a base gained: E = 1)
    want = pref._records(eref.distances(profile, a, b, rc), k, rc, False, False)
    assert set(range(250, n_a)) <= set(want["a_idx"].tolist())
    s = sassy.Searcher(profile, rc=rc)
    for chunks in (0, 2):
        s.set_option("pairs_chunks", chunks)
        check_pairs(s.edit_pairs(a, b, k), want)
        check_nearest(s.edit_nearest(a, b, k), pref.nearest_of_pairs(want, n_a))
    own = eref.distances(profile, a, a, rc)
    check_pairs(s.edit_pairs(a, None, k), pref._records(own, k, rc, True, False))
    check_nearest(s.edit_nearest(a, None, k), pref.nearest_of_pairs(pref._records(own, k, rc, True, True), n_a))


@pytest.mark.parametrize("profile", ("dna", "iupac"))
def test_self_mode_triangle_with_rc(sassy, profile):
    """strand 0 only for i < j, strand 1 for i <= j; a reverse-complement palindrome keeps (i, i, 1) at cost 0; neighbours
    one shift apart, a later entry's reverse complement, a copy with a base lost; nearest sees the full square without
    (i, i, 0)"""
    rng = np.random.default_rng(5)
    m, k, n = 16, 2, 200
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    a = bases[rng.integers(4, size=(n, m))]
    palindromes = (0, 63, 64, 130, n - 1)
    for i in palindromes:
        half = a[i, :m // 2].tobytes()
        a[i] = np.frombuffer(half + oracle.reverse_complement(profile, half), dtype=np.uint8)
    shifted = (1, 65, 131)
    for i in shifted:
        a[i] = np.roll(a[i - 1], 1)
    for i in (2, 66, 132):  # a later entry's reverse complement, and a copy with a base lost
        a[i] = np.frombuffer(oracle.reverse_complement(profile, a[i + 20].tobytes()), dtype=np.uint8)
        a[i + 1, :m - 1], a[i + 1, m - 1] = a[i + 21, 1:], a[i + 21, 0]
    a = np.ascontiguousarray(a)
    table = eref.distances(profile, a, a, True)
    want = pref._records(table, k, True, True, False)
    tuples = set(eref.as_tuples(want))
    for i in palindromes:
        assert (i, i, 1, 0) in tuples
    for i in shifted:
        assert table[i - 1, i, 0] <= 2 and (i - 1, i, 0, int(table[i - 1, i, 0])) in tuples
    for i in (2, 66, 132):
        assert (i, i + 20, 1, 0) in tuples and (i + 1, i + 21, 0, 2) in tuples
    assert not any(i > j or (i == j and s == 0) for i, j, s, _ in tuples)
    s = sassy.Searcher(profile, rc=True)
    check_pairs(s.edit_pairs(a, None, k), want)
    check_nearest(s.edit_nearest(a, None, k), pref.nearest_of_pairs(pref._records(table, k, True, True, True), n))
    # two-set mode of the list against itself is the square, the diagonal's strand 0 included
    check_pairs(s.edit_pairs(a, a, k), pref._records(table, k, True, False, False))
