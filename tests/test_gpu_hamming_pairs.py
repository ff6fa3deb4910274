"""Searcher.hamming_pairs / hamming_nearest on the device against tests/helpers/hamming_pairs_ref.py (a numpy brute force
built from the oracle's relation): records compared for exact equality, array to array, order included.  The sizes are the
smallest at which the kernels can go wrong -- the seams of a wavefront (64 entries), of a strip (256), of a chunk of targets,
the last partial ones, the diagonal of self mode -- not a workload."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import oracle  # noqa: E402
import hamming_ref as href  # noqa: E402
import hamming_pairs_ref as pref  # noqa: E402
from scan_levels import LETTERS, near_copy, random_rows  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 600)
MS = (1, 16, 31, 32, 33, 64, 65, 128)
ALPHABETS = (("dna", False), ("dna", True), ("iupac", False), ("iupac", True), ("ascii", False), ("ascii_ci", False))
KS = (0, 1, 3)
CHUNKS = (0, 1, 2, 3, 7)


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


def seams(n, chunk=None):
    """first and last entry of a wavefront and of a strip, of a chunk of targets, the list's own ends"""
    at = {0, 1, 62, 63, 64, 65, 127, 128, 254, 255, 256, 257, 511, 512, n - 2, n - 1}
    if chunk:
        for c in range(0, n, chunk):
            at |= {c - 1, c, c + 1}
    return sorted(i for i in at if 0 <= i < n)


def chunk_len(n_a, n_b, chunks):
    """targets per chunk; chunks == 0: the planner's own choice (pairs_step.h: pairs_plan -- enough chunks of at least 256
    targets that 2048 workgroups of 256 entries are in flight; at these sizes no other of its bounds binds)"""
    if not chunks:
        chunks = min(-(-2048 // -(-n_a // 256)), max(1, n_b // 256))
    return -(-n_b // min(chunks, n_b))


def plant(rng, profile, rc, a, b, k, chunk, self_mode):
    """near-copies of one sequence, at distances 0 .. k + 1 from each other, on both sides of every seam of a and of b; an
    rc searcher gets some of them as reverse complements; self mode gets them next to the diagonal, and palindromes"""
    m = a.shape[1]
    base = random_rows(rng, "dna", 1, m)[0]  # (plain bases: an Iupac X would match nothing, itself included)
    for q, i in enumerate(seams(len(a), chunk if self_mode else None)):
        a[i] = near_copy(rng, profile, base, q % (k + 2) if self_mode else q % 2 if k else 0)
        if rc and q % 4 == 3:
            a[i] = np.frombuffer(oracle.reverse_complement(profile, a[i].tobytes()), dtype=np.uint8)
    if self_mode:
        if rc and m % 2 == 0:  # reverse-complement palindromes: (i, i, 1) at cost 0
            for i in (2, len(a) // 2, len(a) - 3):
                if 0 <= i < len(a):
                    half = random_rows(rng, "dna", 1, m // 2)[0].tobytes()
                    a[i] = np.frombuffer(half + oracle.reverse_complement(profile, half), dtype=np.uint8)
        return
    for q, j in enumerate(seams(len(b), chunk)):
        b[j] = near_copy(rng, profile, base, q % (k + 2))
        if rc and q % 3 == 2:
            b[j] = np.frombuffer(oracle.reverse_complement(profile, b[j].tobytes()), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def border_case(t, self_mode):
    profile, rc = ALPHABETS[t % 6]
    m = MS[(t // 6) % 8]
    k = KS[(t + t // 6) % 3]
    chunks = CHUNKS[(t + t // 8) % 5]
    n_a = SIZES[(t + t // 6) % 8]
    n_b = SIZES[(3 * t + t // 8 + 1) % 8]
    rng = np.random.default_rng(1000 + 2 * t + self_mode)
    a = random_rows(rng, profile, n_a, m)
    b = None if self_mode else random_rows(rng, profile, n_b, m)
    plant(rng, profile, rc, a, b, k, chunk_len(n_a, n_a if self_mode else n_b, chunks), self_mode)
    want_pairs = pref.expected_pairs(profile, a, b, k, rc)
    want_nearest = pref.expected_nearest(profile, a, b, k, rc)
    return profile, rc, m, k, chunks, a, b, want_pairs, want_nearest


# ---------------------------------------------------------------- (1) borders
@pytest.mark.parametrize("t", range(48))
def test_borders_two_sets(sassy, t):
    """every alphabet and strand setting x every length of the issue's list, the sizes, k and the forced chunk counts cycling
    through their lists: 48 cases cover every kernel instantiation (planes x words) with every chunk count"""
    profile, rc, m, k, chunks, a, b, want_pairs, want_nearest = border_case(t, False)
    s = sassy.Searcher(profile, rc=rc)
    s.set_option("pairs_chunks", chunks)
    got = s.hamming_pairs(a, b, k)
    print(f"case {t}: {profile} rc={rc} m={m} k={k} chunks={chunks} n_a={len(a)} n_b={len(b)} records={len(got)} want={len(want_pairs)}")
    check_pairs(got, want_pairs)
    assert len(want_pairs) > 0
    check_nearest(s.hamming_nearest(a, b, k), want_nearest)
    # lists of bytes give the same as arrays
    if len(a) <= 65:
        check_pairs(s.hamming_pairs([r.tobytes() for r in a], [r.tobytes() for r in b], k), want_pairs)


@pytest.mark.parametrize("t", range(48))
def test_borders_self_mode(sassy, t):
    """the triangle: strand 0 for i < j, strand 1 for i <= j, plants on and next to the diagonal, palindromes for (i, i, 1);
    nearest sees the full square without (i, i, 0); every alphabet and strand setting at every length"""
    profile, rc, m, k, chunks, a, _, want_pairs, want_nearest = border_case(t, True)
    s = sassy.Searcher(profile, rc=rc)
    s.set_option("pairs_chunks", chunks)
    got = s.hamming_pairs(a, None, k)
    print(f"case {t}: {profile} rc={rc} m={m} k={k} chunks={chunks} n={len(a)} records={len(got)} want={len(want_pairs)}")
    check_pairs(got, want_pairs)
    assert (got["a_idx"] <= got["b_idx"]).all() and (got["a_idx"][got["strand"] == 0] < got["b_idx"][got["strand"] == 0]).all()
    check_nearest(s.hamming_nearest(a, None, k), want_nearest)


def test_self_mode_diagonal_by_hand(sassy):
    """the hand-written case of the helper, on the device; GAATTC and ACGT are their own reverse complements"""
    for rc, pairs, nearest in ((True, pref.HAND_SELF_PAIRS_RC, pref.HAND_SELF_NEAREST_RC), (False, pref.HAND_SELF_PAIRS_FWD, pref.HAND_SELF_NEAREST_FWD)):
        s = sassy.Searcher("dna", rc=rc)
        assert pref.as_tuples(s.hamming_pairs(pref.HAND_SELF, None, pref.HAND_K)) == pairs
        cols = s.hamming_nearest(pref.HAND_SELF, None, pref.HAND_K)
        assert [tuple(int(c[i]) for c in cols) for i in range(4)] == nearest
    s = sassy.Searcher("dna", rc=False)
    assert pref.as_tuples(s.hamming_pairs(pref.HAND_A, pref.HAND_B, pref.HAND_K)) == pref.HAND_TWO_PAIRS
    s = sassy.Searcher("iupac", rc=True)
    seqs = [b"GAATTC", b"GAATTC", b"CCCCCC"]
    assert pref.as_tuples(s.hamming_pairs(seqs, None, 0)) == [(0, 0, 1, 0), (0, 1, 0, 0), (0, 1, 1, 0), (1, 1, 1, 0)]


# ---------------------------------------------------------------- (2) dense, (3) empty
def test_dense_every_pair_is_a_record(sassy):
    """k >= m: every (i, j, strand) is a record -- 180 000 of them, the complete order checked; the self-mode triangle holds
    exactly n (n - 1) / 2 strand-0 and n (n + 1) / 2 strand-1 records"""
    rng = np.random.default_rng(7)
    n, m = 300, 4
    a, b = random_rows(rng, "dna", n, m), random_rows(rng, "dna", n, m)
    s = sassy.Searcher("dna", rc=True)
    for chunks in (0, 3):
        s.set_option("pairs_chunks", chunks)
        got = s.hamming_pairs(a, b, 9)
        assert len(got) == 2 * n * n == 180000
        i, j, st = np.meshgrid(np.arange(n), np.arange(n), np.arange(2), indexing="ij")
        assert (got["a_idx"] == i.ravel()).all() and (got["b_idx"] == j.ravel()).all() and (got["strand"] == st.ravel()).all()
        assert (got["cost"] == pref.distances("dna", a, b, True).ravel()).all()
        tri = s.hamming_pairs(a, None, m)
        assert int((tri["strand"] == 0).sum()) == n * (n - 1) // 2 and int((tri["strand"] == 1).sum()) == n * (n + 1) // 2
        check_pairs(tri, pref.expected_pairs("dna", a, None, m, True))
    cost, index, strand, ties = s.hamming_nearest(a, b, m)
    check_nearest((cost, index, strand, ties), pref.expected_nearest("dna", a, b, m, True))


def test_empty_result_is_valid(sassy):
    rng = np.random.default_rng(11)
    rows = np.unique(random_rows(rng, "dna", 1200, 32), axis=0)
    rows = rows[rng.permutation(len(rows))]
    a, b = rows[:500], rows[500:1000]
    assert len(b) == 500
    s = sassy.Searcher("dna", rc=False)
    for second in (b, None):
        got = s.hamming_pairs(a, second, 0)
        assert len(got) == 0 and got.dtype == sassy.hamming_pair_dtype()
        cost, index, strand, ties = s.hamming_nearest(a, second, 0)
        assert (cost == sassy.NO_MATCH).all() and (index == 0xFFFFFFFF).all() and not strand.any() and not ties.any()
    # the searcher still serves the family's other calls afterwards
    text = b"TTTT" + a[0].tobytes() + b"GGGG"
    assert [href.key(x) for x in s.search_hamming(a[0].tobytes(), text, 1)] == [href.key(x) for x in href.expected("dna", a[0].tobytes(), text, 1)]


# ---------------------------------------------------------------- (4) the relations
def test_iupac_sets_and_pad_bits(sassy):
    s = sassy.Searcher("iupac", rc=False)
    for m in (33, 65):  # all N: every row matches; the pad bits of the last word neither match nor mismatch
        got = s.hamming_pairs([b"N" * m, b"A" * m], [b"N" * m, b"C" * m], 0)
        assert pref.as_tuples(got) == [(0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0)]
        cost, _, _, _ = s.hamming_nearest([b"N" * m], [b"N" * m], 0)
        assert cost.tolist() == [0]
        # disjoint sets cost one per row: exactly m, the pad bits add nothing
        cost, _, _, ties = s.hamming_nearest([b"A" * m], [b"C" * m, b"G" * m], 128)
        assert cost.tolist() == [m] and ties.tolist() == [2]
    assert pref.as_tuples(s.hamming_pairs([b"NNNN", b"ACGT"], [b"ACGT", b"RYKM"], 1)) == [(0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 0, 1)]
    assert pref.as_tuples(s.hamming_pairs([b"AAAA"], [b"ACAA", b"CCAA", b"XAAA"], 1)) == [(0, 0, 0, 1), (0, 2, 0, 1)]


def test_dna_follows_the_two_bit_code(sassy):
    """lower case and other bytes: (c >> 1) & 3, as the family does"""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, size=(70, 20), dtype=np.uint8)
    b = a.copy()[::-1] ^ rng.choice(np.array([0, 0, 0, 1, 0x20, 0x81, 2, 4], dtype=np.uint8), size=a.shape)
    for rc in (False, True):
        s = sassy.Searcher("dna", rc=rc)
        check_pairs(s.hamming_pairs(a, b, 6), pref.expected_pairs("dna", a, b, 6, rc))
    s = sassy.Searcher("dna", rc=False)
    assert pref.as_tuples(s.hamming_pairs([b"acgt"], [b"ACGT", b"ACGU", b"ACGG"], 0)) == [(0, 0, 0, 0), (0, 1, 0, 0)]
    c = sassy.Searcher("ascii_ci", rc=False)
    assert pref.as_tuples(c.hamming_pairs([b"abc@"], [b"ABC@", b"ABC`", b"abc@"], 0)) == [(0, 0, 0, 0), (0, 2, 0, 0)]
    assert pref.as_tuples(sassy.Searcher("ascii", rc=False).hamming_pairs([b"abc@"], [b"ABC@", b"abc@"], 0)) == [(0, 1, 0, 0)]


# ---------------------------------------------------------------- (5) nearest
def test_nearest_ties_and_tie_rule(sassy):
    m = 24
    x = b"ACGTTGCAAGGCTTAACCGGATAT"
    far = b"T" * m
    one = bytearray(x); one[5] = ord("A")
    two = bytearray(x); two[5] = ord("A"); two[9] = ord("C")
    rcx = oracle.reverse_complement("dna", x)
    b = [far] * 600
    b[10], b[590], b[300] = bytes(one), bytes(one), bytes(two)  # a tie at cost 1 across the chunks of 2, 3 and 7
    for rc in (False, True):
        s = sassy.Searcher("dna", rc=rc)
        for chunks in (0, 1, 2, 3, 7):
            s.set_option("pairs_chunks", chunks)
            cost, index, strand, ties = s.hamming_nearest([x, far, bytes(two)], b, 1)
            assert cost.tolist() == [1, 0, 0] and index.tolist() == [10, 0, 300] and strand.tolist() == [0, 0, 0]
            assert ties.tolist() == [2, 597, 1]
            # the cap at k
            cost, index, strand, ties = s.hamming_nearest([x], [far, bytes(two)], 1)
            assert (cost.tolist(), index.tolist(), strand.tolist(), ties.tolist()) == ([sassy.NO_MATCH], [0xFFFFFFFF], [0], [0])
            cost, index, _, ties = s.hamming_nearest([x], [far, bytes(two)], 2)
            assert (cost.tolist(), index.tolist(), ties.tolist()) == ([2], [1], [1])
    # the same target on both strands: Fwd first; a reverse complement at a lower index beats a forward copy behind it
    s = sassy.Searcher("dna", rc=True)
    pal = b"ACGTACGTACGTACGTACGTACGT"
    cost, index, strand, ties = s.hamming_nearest([pal, x], [far, pal, rcx, x], 0)
    assert (cost.tolist(), index.tolist(), strand.tolist(), ties.tolist()) == ([0, 0], [1, 2], [0, 1], [2, 2])
    # A entries in different strips see the same
    a = [far] * 600
    a[0], a[255], a[256], a[599] = x, x, x, x
    for chunks in (0, 7):
        s.set_option("pairs_chunks", chunks)
        cost, index, strand, ties = s.hamming_nearest(a, b + [rcx], 1)
        for i in (0, 255, 256, 599):
            assert (cost[i], index[i], strand[i], ties[i]) == (0, 600, 1, 1)


def test_nearest_self_mode_excludes_only_itself_forward(sassy):
    rng = np.random.default_rng(3)
    a = random_rows(rng, "dna", 300, 20)
    a[7] = a[3]
    a[299] = a[0]
    half = a[50][:10].tobytes()
    a[50] = np.frombuffer(half + oracle.reverse_complement("dna", half), dtype=np.uint8)  # its own reverse complement
    for rc in (False, True):
        s = sassy.Searcher("dna", rc=rc)
        for chunks in (0, 2, 7):
            s.set_option("pairs_chunks", chunks)
            got = s.hamming_nearest(a, None, 4)
            check_nearest(got, pref.expected_nearest("dna", a, None, 4, rc))
            cost, index, strand, ties = got
            assert (cost[3], index[3], cost[7], index[7], cost[0], index[0], index[299]) == (0, 7, 0, 3, 0, 299, 0)
            if rc:
                assert (cost[50], index[50], strand[50]) == (0, 50, 1)
            else:
                assert index[50] != 50


def test_nearest_is_the_reduction_of_pairs(sassy):
    rng = np.random.default_rng(17)
    for profile, rc in ALPHABETS:
        a, b = random_rows(rng, profile, 257, 12), random_rows(rng, profile, 300, 12)
        s = sassy.Searcher(profile, rc=rc)
        s.set_option("pairs_chunks", 3)
        for second, k in ((b, 5), (None, 5)):
            pairs = s.hamming_pairs(a, second, k)
            if second is None:  # the triangle mirrored into the square nearest sees: (i, j, s) also as (j, i, s), once
                off = pairs[pairs["a_idx"] != pairs["b_idx"]]
                mirror = off.copy()
                mirror["a_idx"], mirror["b_idx"] = off["b_idx"], off["a_idx"]
                pairs = np.concatenate([pairs, mirror])
                pairs = pairs[np.lexsort((pairs["strand"], pairs["b_idx"], pairs["a_idx"]))]
            check_nearest(s.hamming_nearest(a, second, k), pref.nearest_of_pairs(pairs, len(a)))


# ---------------------------------------------------------------- (6) the existing path, determinism
def test_cross_check_with_hamming_best_pattern(sassy):
    """reads of exactly m bytes: the new call and the sliding one answer the same (cost, index, strand)"""
    rng = np.random.default_rng(23)
    m, k = 20, 2
    for profile, rc in (("dna", False), ("dna", True), ("iupac", False), ("iupac", True)):
        barcodes = random_rows(rng, profile, 96, m)
        reads = random_rows(rng, "dna", 500, m)
        for i in range(0, 500, 2):  # half the reads: a barcode, or its reverse complement, with 0 .. 3 changes
            src = barcodes[rng.integers(0, 96)].tobytes()
            if i % 4 == 2:
                src = oracle.reverse_complement(profile, src)
            reads[i] = near_copy(rng, "dna", np.frombuffer(src, dtype=np.uint8), (i // 4) % 4)
        s = sassy.Searcher(profile, rc=rc)
        cost, index, strand, _ = s.hamming_nearest(reads, barcodes, k)
        old_cost, old_pattern, old_strand, _ = s.hamming_best_pattern([r.tobytes() for r in barcodes], [r.tobytes() for r in reads], k)
        assert cost.tolist() == old_cost.tolist() and index.tolist() == old_pattern.tolist() and strand.tolist() == old_strand.tolist()
        # (the inputs are no degenerate case: of the 125 forward copies, 94 carry at most k changes; an Iupac barcode's X rows
        # cost one each on top, which leaves 63 of them)
        assert (cost != sassy.NO_MATCH).sum() >= 60
        check_nearest((cost, index, strand), pref.expected_nearest(profile, reads, barcodes, k, rc)[:3])


def test_same_call_twice_gives_the_same_bytes(sassy):
    rng = np.random.default_rng(29)
    a, b = random_rows(rng, "dna", 600, 8), random_rows(rng, "dna", 257, 8)
    s = sassy.Searcher("dna", rc=True)
    s.set_option("pairs_chunks", 7)
    first = s.hamming_pairs(a, b, 2)
    assert len(first) > 500 and first.tobytes() == s.hamming_pairs(a, b, 2).tobytes()
    assert first.tobytes() == sassy.Searcher("dna", rc=True).hamming_pairs(a, b, 2).tobytes()  # (another geometry too)
    n1, n2 = s.hamming_nearest(a, None, 2), s.hamming_nearest(a, None, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(n1, n2))
    st = s.stats()
    assert st["filtered"] == 8 and st["chunks"] == 7


# ---------------------------------------------------------------- (7) the `pairs` verb
def test_cli_pairs_rows(sassy, tmp_path, capsys):
    from sassy_amd import cli
    a = tmp_path / "a.txt"
    a.write_bytes(b"\n".join(pref.HAND_SELF) + b"\n")
    b = tmp_path / "b.fa"
    b.write_bytes(b">w1\nACGA\n>w2 second\nACGT\n>w3\nCCCC\n")
    assert cli.main(["pairs", str(a), "-k", "1", "--rc"]) == 0
    assert capsys.readouterr().out == "a_id\tb_id\tstrand\tcost\n1\t1\t-\t0\n1\t2\t+\t1\n1\t2\t-\t1\n3\t4\t-\t1\n"
    assert cli.main(["pairs", str(a), str(b), "-k", "1", "--nearest"]) == 0
    assert capsys.readouterr().out == ("a_id\tb_id\tstrand\tcost\tties\n1\tw2 second\t+\t0\t1\n2\tw1\t+\t0\t1\n3\t*\t*\t-1\t0\n4\t*\t*\t-1\t0\n")


# ---------------------------------------------------------------- (8) open tickets
def test_open_tickets_refuse_both_calls(sassy):
    """the last of the family's checks: a searcher with a search in flight refuses both calls, in two-set and in self mode,
    with SASSY_HIP_EINVAL and the family's message, and serves them again once the ticket is finished"""
    rng = np.random.default_rng(31)
    text = random_rows(rng, "dna", 1, 5000)[0].tobytes()
    a = [text[100:120], text[300:320], text[100:120]]
    b = [text[300:320], text[500:520]]
    buf = sassy.DeviceBuffer(len(text) + 64)
    buf.upload(text)
    for rc in (False, True):
        s = sassy.Searcher("dna", rc=rc)
        ticket = s.search_shard_begin(text[100:120], buf.ptr, 0, len(text), 0, len(text), 1)
        for call in (lambda: s.hamming_pairs(a, b, 1), lambda: s.hamming_pairs(a, None, 1),
                     lambda: s.hamming_nearest(a, b, 1), lambda: s.hamming_nearest(a, None, 1)):
            with pytest.raises(sassy.SassyHipError, match=r"error -1: searches are in flight on this searcher"):
                call()
        assert len(s.search_finish(ticket).matches) >= 1
        check_pairs(s.hamming_pairs(a, b, 1), pref.expected_pairs("dna", a, b, 1, rc))
        check_pairs(s.hamming_pairs(a, None, 1), pref.expected_pairs("dna", a, None, 1, rc))
        check_nearest(s.hamming_nearest(a, b, 1), pref.expected_nearest("dna", a, b, 1, rc))
        check_nearest(s.hamming_nearest(a, None, 1), pref.expected_nearest("dna", a, None, 1, rc))
        assert pref.as_tuples(s.hamming_pairs(a, None, 0))[:1] == [(0, 2, 0, 0)]
    buf.free()
