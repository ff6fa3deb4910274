"""The paired-end overlap call on the device (sassy_amd/csrc/read_overlaps.hip) against its definition
(tests/helpers/read_overlaps_ref.py), array against array, no tolerance anywhere.

Geometry the shapes aim at: one wavefront per pair, four pairs per workgroup; 64 bytes per ballot step; the lanes as offsets,
64 per round; plane words of 32 rows, b's shifted by a word index and a bit count per lane; the kernel is instantiated for
2, 4, 6, 8 and 16 words per plane, picked by the longest read of BOTH batches (64, 128, 192, 256, 512 bytes) -- `word_rows`
of the call's stats says which one ran.  The shapes are the smallest at which these can go wrong, not a workload."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import read_overlaps_ref as oref  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 150, 191, 192, 193, 511, 512)
WORDS = {64: 2, 128: 4, 192: 6, 256: 8, 512: 16}


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


@pytest.fixture(scope="module")
def searchers(sassy):
    return {"dna": sassy.Searcher("dna", rc=False), "iupac": sassy.Searcher("iupac", rc=False)}


def check(searchers, profile, r1s, r2s, ctx, words=None, **kw):
    """the call over lists (DeviceReads.from_sequences) against the helper, record by record"""
    s = searchers[profile]
    got = s.read_overlaps(r1s, r2s, **kw)
    want = oref.expected_overlaps(profile, r1s, r2s, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape, ctx
    bad = np.flatnonzero(got != want)
    assert not bad.size, (ctx, profile, kw, "pair", int(bad[0]), "of", len(want), "lengths", len(r1s[int(bad[0])]), len(r2s[int(bad[0])]),
                          "got", got[bad[0]].tolist(), "want", want[bad[0]].tolist())
    if words is not None and len(r1s):
        assert s.stats()["word_rows"] == words, (ctx, s.stats()["word_rows"], words)
    return got


def fastq_of(seqs, tag=b"r"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def random_seq(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), n).astype(np.uint8)) if n else b""


# ---------------------------------------------------------------- the cases written out by hand
def test_the_two_hand_cases(sassy, searchers):
    for profile in ("dna", "iupac"):
        for case in oref.HAND:
            got = check(searchers, profile, [case["r1"]], [case["r2"]], "hand", words=2, min_overlap=case["min_overlap"], k=0, max_permille=0)
            assert tuple(got[0].tolist()) == case["record"]
            assert sassy.overlap_trims(got[0], len(case["r1"]), len(case["r2"])) == case["trims"]


# ---------------------------------------------------------------- lengths
@pytest.mark.parametrize("profile", ["dna", "iupac"])
def test_every_pair_of_lengths_with_a_planted_overlap(searchers, profile):
    """Every (la, lb) of LENGTHS squared, once per instantiation that can hold it: a random fragment with a planted true
    overlap (as long as the shorter read allows, at most 40 rows) and one or two substitutions in it."""
    rng = np.random.default_rng(11)
    for cap, words in WORDS.items():
        lengths = [n for n in LENGTHS if n <= cap]  # (the longest of them picks this instantiation)
        r1s, r2s = [], []
        for la in lengths:
            for lb in lengths:
                ov = min(la, lb, 40)
                d = la - ov if (la + lb) % 2 == 0 or la < ov else -(lb - ov)  # ordinary overlap / read-through, by turns
                a, r2 = oref.planted_pair(rng, profile, la, lb, d if la and lb else 0, subs=1 + (la + lb) % 2 if ov >= 12 else 0)
                r1s.append(a)
                r2s.append(r2)
        got = check(searchers, profile, r1s, r2s, ("lengths", cap), words=words, min_overlap=5, k=4, max_permille=250)
        assert (got["n_accepted"] > 0).sum() >= sum(1 for x, y in zip(r1s, r2s) if min(len(x), len(y)) >= 12), cap


# ---------------------------------------------------------------- best offset at the seams and the extremes
def test_best_offset_at_the_word_seams_and_at_the_outermost_offsets(searchers):
    rng = np.random.default_rng(12)
    la = lb = 150
    mo = 12
    r1s, r2s, want_d = [], [], []
    for d in (-65, -64, -63, -33, -32, -31, -1, 0, 1, 31, 32, 33, 63, 64, 65, la - mo, -(lb - mo)):
        a, r2 = oref.planted_pair(rng, "dna", la, lb, d)
        r1s.append(a); r2s.append(r2); want_d.append(d)
    for profile in ("dna", "iupac"):
        got = check(searchers, profile, r1s, r2s, "seams", words=6, min_overlap=mo, k=0, max_permille=0)
        assert got["offset"].tolist() == want_d and (got["mismatches"] == 0).all()
        assert got["overlap"].tolist() == [min(la, d + lb) - max(0, d) for d in want_d]
    # one offset further out overlaps in min_overlap - 1 rows: not accepted, although it matches exactly
    r1s, r2s = zip(*(oref.planted_pair(rng, "dna", la, lb, d) for d in (la - mo + 1, -(lb - mo + 1))))
    got = check(searchers, "dna", list(r1s), list(r2s), "one further out", min_overlap=mo, k=0, max_permille=0)
    assert got.tolist() == [(0, 0, 0, 0)] * 2
    got = check(searchers, "dna", list(r1s), list(r2s), "one further out, one row less asked", min_overlap=mo - 1, k=0, max_permille=0)
    assert got["offset"].tolist() == [la - mo + 1, -(lb - mo + 1)] and got["overlap"].tolist() == [mo - 1] * 2
    # the outermost offsets of all: one row of overlap, at both ends, reads of 512
    # (b = A G...G under a = C...C A meets it in its last row only; mirrored for the other end)
    got = check(searchers, "dna", [b"C" * 511 + b"A", b"A" + b"C" * 511], [b"C" * 511 + b"T", b"T" + b"C" * 511], "one row", words=16, min_overlap=1,
                k=0, max_permille=0)
    assert got.tolist() == [(511, 1, 0, 1), (-511, 1, 0, 1)]


# ---------------------------------------------------------------- exact ties
def test_exact_ties_and_thresholds(searchers):
    rng = np.random.default_rng(13)

    def flip(seq, positions):
        swap = {65: 67, 67: 71, 71: 84, 84: 65}
        out = bytearray(seq)
        for p in positions:
            out[p] = swap[out[p]]
        return bytes(out)

    L = 100
    # d and -d with the same overlap and no mismatch: a = S M T, b = T M' S -- the larger d wins
    S, M, M2, T = (random_seq(rng, n) for n in (30, 40, 40, 30))
    a, b = S + M + T, T + M2 + S
    got = check(searchers, "dna", [a], [oref.revcomp("dna", b)], "mirror", min_overlap=20, k=0, max_permille=0)
    assert got.tolist() == [(L - 30, 30, 0, 2)]
    # equal density at different overlaps, 1/20 against 2/40: the longer overlap wins; 50 per thousand is met exactly by both
    S, M, M2, T = (random_seq(rng, n) for n in (20, 40, 40, 40))
    a, b = S + M + T, flip(T, (3, 17)) + M2 + flip(S, (9,))
    got = check(searchers, "dna", [a], [oref.revcomp("dna", b)], "density tie", min_overlap=20, k=2, max_permille=50)
    assert got.tolist() == [(L - 40, 40, 2, 2)]
    # ... one more mismatch in the long one: 3/40 is over 50 per thousand, the short one is left alone
    b3 = flip(T, (3, 17, 30)) + M2 + flip(S, (9,))
    got = check(searchers, "dna", [a], [oref.revcomp("dna", b3)], "over the permille", min_overlap=20, k=3, max_permille=50)
    assert got.tolist() == [(-(L - 20), 20, 1, 1)]
    # mm * 1000 == max_permille * ov exactly is accepted, one per thousand less is not
    got = check(searchers, "dna", [a], [oref.revcomp("dna", b)], "permille - 1", min_overlap=20, k=2, max_permille=49)
    assert got.tolist() == [(0, 0, 0, 0)]
    # mm == k is accepted, k + 1 mismatches are not
    got = check(searchers, "dna", [a], [oref.revcomp("dna", b)], "k below", min_overlap=20, k=1, max_permille=1000)
    assert got.tolist() == [(-(L - 20), 20, 1, 1)]
    got = check(searchers, "dna", [a], [oref.revcomp("dna", b)], "k == mm", min_overlap=20, k=2, max_permille=100)
    assert got.tolist() == [(L - 40, 40, 2, 2)]
    # k is not capped at 254: 300 mismatches in 512 rows
    a = random_seq(rng, 512)
    b = flip(a, range(0, 300))
    for k, want in ((299, (0, 0, 0, 0)), (300, (0, 512, 300, 1)), (1 << 40, (0, 512, 300, 1))):
        got = check(searchers, "dna", [a], [oref.revcomp("dna", b)], ("k", k), words=16, min_overlap=512, k=k, max_permille=1000)
        assert got.tolist() == [want]


# ---------------------------------------------------------------- n_accepted
def test_accepted_counts_of_low_complexity_reads(searchers):
    mo = 8
    got = check(searchers, "dna", [b"A" * 30, b"A" * 30, b"A" * 20], [b"T" * 30, b"T" * 20, b"T" * 30], "poly-A", min_overlap=mo, k=0, max_permille=0)
    # every offset from min_overlap rows up is accepted; the longest overlap wins, and among equals the larger d
    assert got.tolist() == [(0, 30, 0, 2 * (30 - mo) + 1), (10, 20, 0, 30 + 20 - 2 * mo + 1), (0, 20, 0, 30 + 20 - 2 * mo + 1)]
    unit = b"ACGGCCGT"  # (a tandem repeat whose unit is its own reverse complement: every shift by the unit matches)
    assert oref.revcomp("dna", unit) == unit
    got = check(searchers, "dna", [unit * 8], [unit * 8], "tandem", min_overlap=mo, k=0, max_permille=0)
    assert got[0]["n_accepted"] == 2 * 7 + 1 and got[0]["offset"] == 0 and got[0]["overlap"] == 64
    got = check(searchers, "dna", [unit * 8 + b"AC"], [unit * 20], "tandem, two lengths", words=6, min_overlap=mo, k=1, max_permille=100)
    assert got[0]["n_accepted"] > 3


# ---------------------------------------------------------------- Iupac, and what a Dna searcher refuses
def test_iupac_letters_and_the_dna_refusal(sassy, searchers):
    rng = np.random.default_rng(14)
    letters = b"ACGTNUacgtnuRYKMSWBDHVX-*"
    r1s = [random_seq(rng, n, letters) for n in (40, 150, 64, 33, 200)]
    r2s = [random_seq(rng, n, letters) for n in (40, 150, 65, 90, 130)]
    for i in (0, 1, 4):  # a true overlap under the complement of every letter
        b = oref.revcomp("iupac", r2s[i])
        r2s[i] = oref.revcomp("iupac", r1s[i][-20:] + b[20:])
    got = check(searchers, "iupac", r1s, r2s, "iupac letters", words=8, min_overlap=10, k=10, max_permille=300)
    assert (got["n_accepted"] > 0).any()
    # U matches as T and stays U under the complement; X matches nothing, itself included; a non-letter matches as N
    got = check(searchers, "iupac", [b"TTTTA", b"XXXXX", b"ACGT-"], [b"NUUUU", b"XXXXX", b"*ACGT"], "U X *", words=2, min_overlap=5, k=0, max_permille=0)
    assert got.tolist() == [(0, 5, 0, 1), (0, 0, 0, 0), (0, 5, 0, 1)]
    # the same reads under dna: refused, whichever batch holds the letter, with the way out in the message
    for x, y, who in ((r1s, [b"ACGT"] * 5, "r1"), ([b"ACGT"] * 5, r2s, "r2"), ([b"ACGN"], [b"ACGT"], "r1"), ([b"ACGT"], [b"AC-T"], "r2")):
        with pytest.raises(sassy.SassyHipError, match=who + " holds other bytes than A, C, G, T.*iupac searcher"):
            searchers["dna"].read_overlaps(x, y)
    # lower-case a, c, g, t pass the look (as for every _reads call) and count as the definition counts them
    check(searchers, "dna", [b"ACGTacgtACGTacgt", b"acgtacgtacgtacgg"], [b"acgtACGTacgtACGT", b"ccgtacgtacgtacgt"], "lower case", min_overlap=4, k=2, max_permille=200)


# ---------------------------------------------------------------- different layouts in the two handles
def test_layouts_differ_between_the_handles(sassy, searchers):
    rng = np.random.default_rng(15)
    for n in (1, 63, 65, 1025):
        r1s = [random_seq(rng, 150) for _ in range(n)]
        r2s = []
        for i, a in enumerate(r1s):
            lb = int(rng.integers(40, 301))
            b = bytearray(random_seq(rng, lb))
            ov = min(lb, 150, int(rng.integers(10, 120)))
            b[:ov] = a[150 - ov:]  # (d = 150 - ov)
            for p in rng.integers(0, ov, 2 if i % 3 == 0 else 0).tolist():
                b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1) % 4]
            r2s.append(oref.revcomp("dna", bytes(b)))
        for at in {0, n // 2, n - 1}:  # empty reads at the first, a middle and the last position, by turns in either file
            if at % 2:
                r1s[at] = b""
            else:
                r2s[at] = b""
        profile = "dna" if n != 65 else "iupac"
        got = check(searchers, profile, r1s, r2s, ("layouts", n), min_overlap=10, k=20, max_permille=200)
        assert (got["n_accepted"] == 0).sum() >= len({0, n // 2, n - 1})
        assert n < 4 or (got["n_accepted"] > 0).sum() >= n - 4


# ---------------------------------------------------------------- several rounds, every instantiation
def test_every_round_count_of_every_instantiation(searchers):
    """la + lb - 1 offsets span 1 .. 16 rounds of 64; each batch's longest read picks one instantiation, and min_overlap = 1
    keeps every offset in the walk.  The true overlap sits in the LAST round's offsets and in the first's by turns."""
    rng = np.random.default_rng(16)
    for cap, words in WORDS.items():
        r1s, r2s = [random_seq(rng, cap)], [random_seq(rng, cap)]   # (the pair that picks the instantiation; 2 * cap / 64 rounds)
        for rounds in range(1, 2 * cap // 64 + 1):
            for offsets in (64 * (rounds - 1) + 1, 64 * rounds):  # the fewest and the most offsets that take this many rounds
                if offsets + 1 > 2 * cap:
                    continue
                la = min(cap, (offsets + 2) // 2)
                lb = offsets + 1 - la
                ov = min(la, lb, 9)
                d = la - ov if rounds % 2 else -(lb - ov)
                a, r2 = oref.planted_pair(rng, "dna", la, lb, d)
                r1s.append(a); r2s.append(r2)
        check(searchers, "dna", r1s, r2s, ("rounds", cap), words=words, min_overlap=1, k=0, max_permille=0)
        check(searchers, "iupac", r1s, r2s, ("rounds", cap), words=words, min_overlap=7, k=1, max_permille=150)


# ---------------------------------------------------------------- the handles
def test_inputs_stay_as_they_were_and_resident_and_list_inputs_agree(sassy, searchers):
    rng = np.random.default_rng(17)
    r1s = [random_seq(rng, int(n)) for n in rng.integers(0, 200, 70)]
    r2s = [oref.revcomp("dna", a[-30:] + random_seq(rng, 40)) if len(a) >= 30 else random_seq(rng, 50) for a in r1s]
    s = searchers["dna"]
    h1, h2 = sassy.DeviceReads(fastq_of(r1s)), sassy.DeviceReads(fastq_of(r2s, b"mate"))
    l1, l2 = sassy.DeviceReads.from_sequences(r1s), sassy.DeviceReads.from_sequences(r2s)
    try:
        before = (h1.download_text(), h2.download_text(), h1.download_rem().tolist(), h2.download_rem().tolist())
        pats = [b"ACGTACGTAC", b"TTTT"]
        key = lambda m: (m.pattern_idx, m.text_idx, m.text_start, m.cost, m.strand, m.cigar)
        hits = [key(m) for m in s.search_hamming_many(pats, h1, 2)]
        got = s.read_overlaps(h1, h2, 10, 5, 200)
        assert [key(m) for m in s.search_hamming_many(pats, h1, 2)] == hits and len(hits) >= 1
        assert (h1.download_text(), h2.download_text(), h1.download_rem().tolist(), h2.download_rem().tolist()) == before
        want = oref.expected_overlaps("dna", r1s, r2s, 10, 5, 200)
        assert np.array_equal(got, want) and (got["n_accepted"] > 0).sum() > 30
        # real FASTQ bytes, from_sequences and plain lists: one result; a second call on the same handles: the same again
        assert np.array_equal(s.read_overlaps(l1, l2, 10, 5, 200), want) and np.array_equal(s.read_overlaps(r1s, r2s, 10, 5, 200), want)
        assert np.array_equal(s.read_overlaps(h1, l2, 10, 5, 200), want) and np.array_equal(s.read_overlaps(h1, h2, 10, 5, 200), want)
        assert [l1.id(0), l1.quality(0), l1.download(3)] == ["", b"", r1s[3]]
        # another searcher on the same handles
        assert np.array_equal(searchers["iupac"].read_overlaps(h1, h2, 10, 5, 200), oref.expected_overlaps("iupac", r1s, r2s, 10, 5, 200))
    finally:
        for h in (h1, h2, l1, l2):
            h.free()


def test_refusals_that_read_the_handles_and_zero_pairs(sassy, searchers):
    s = searchers["dna"]
    assert s.read_overlaps([], []).shape == (0,) and s.read_overlaps([], []).dtype == sassy.read_overlap_dtype()
    with pytest.raises(sassy.SassyHipError, match="r1 holds 2 reads, r2 holds 3"):
        s.read_overlaps([b"ACGT"] * 2, [b"ACGT"] * 3)
    # a read over the limit, in either batch: refused on the host, never launched
    for x, y in (([b"A" * 513, b"ACGT"], [b"ACGT"] * 2), ([b"ACGT"] * 2, [b"ACGT", b"C" * 600])):
        with pytest.raises(sassy.SassyHipError, match="at most 512 bytes"):
            s.read_overlaps(x, y)
    with pytest.raises(sassy.SassyHipError, match="min_overlap must be at least 1"):
        s.read_overlaps([b"ACGT"], [b"ACGT"], min_overlap=0)
    h = sassy.DeviceReads.from_sequences([b"ACGT"])
    import ctypes as C
    rc = sassy.lib().sassy_hip_read_overlaps(s._h, h._handle(), h._handle(), 1, 0, 0, 0, None)
    assert rc == -1 and "must not be null" in sassy.lib().sassy_hip_last_error().decode()
    h.free()
    with pytest.raises(sassy.SassyHipError, match="freed"):
        s.read_overlaps(h, h)
    assert C.sizeof(C.c_int32) * 4 == sassy.read_overlap_dtype().itemsize


# ---------------------------------------------------------------- the reader and the CLI
def test_cli_rows_equal_the_helper_and_unequal_files_raise(sassy, capsys, tmp_path, monkeypatch):
    from sassy_amd import cli, fastx
    rng = np.random.default_rng(18)
    n = 41
    r1s = [random_seq(rng, int(x)) for x in rng.integers(20, 151, n)]
    r2s = []
    for i, a in enumerate(r1s):
        frag = a + random_seq(rng, int(rng.integers(0, 60)))           # ordinary overlap ...
        if i % 3 == 0:
            frag = a[:int(rng.integers(12, len(a)))]                   # ... or a fragment shorter than the read: read-through
        lb = int(rng.integers(20, 151))
        r2s.append(oref.revcomp("dna", frag)[:lb] if i % 3 else oref.revcomp("dna", frag) + random_seq(rng, 10))
    p1, p2 = tmp_path / "r1.fq", tmp_path / "r2.fq"
    p1.write_bytes(fastq_of(r1s, b"pair"))
    p2.write_bytes(fastq_of(r2s, b"mate"))
    want = oref.expected_overlaps("dna", r1s, r2s, 12, 3, 100)
    rows = []
    for i in range(n):
        insert, keep1, keep2 = oref.trims(want[i].tolist(), len(r1s[i]), len(r2s[i]))
        rows.append("pair%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((i,) + tuple(want[i].tolist()) + (insert, keep1, keep2)))
    assert sum(1 for r in want if r["offset"] < 0) >= 5 and sum(1 for r in want if r["offset"] > 0) >= 5
    for batch in (cli.BATCH_BYTES, 1500):  # (the second: many chunks, cut at different records of the two files)
        monkeypatch.setattr(cli, "BATCH_BYTES", batch)
        capsys.readouterr()
        assert cli.main(["overlap", str(p1), str(p2), "--min-overlap", "12", "-k", "3", "--max-permille", "100"]) == 0
        assert capsys.readouterr().out == cli.OVERLAP_HEADER + "".join(rows)
    pairs = list(fastx.read_fastq_pair_device_batches(str(p1), str(p2), 1500))
    assert len(pairs) > 3 and all(len(a) == len(b) for a, b in pairs) and sum(len(a) for a, _ in pairs) == n
    assert pairs[1][0].id(0).startswith("pair") and pairs[1][1].id(0).startswith("mate")
    for a, b in pairs:
        a.free(); b.free()
    p2.write_bytes(fastq_of(r2s[:-1], b"mate"))
    with pytest.raises(ValueError, match="different record counts"):
        cli.main(["overlap", str(p1), str(p2)])
