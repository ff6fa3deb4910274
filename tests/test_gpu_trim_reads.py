"""Adapter and quality trimming on the device (sassy_amd/csrc/trim_reads.hip) and the window call against their definition
(tests/helpers/trim_reads_ref.py, numpy slicing): every comparison is exact equality -- the records, the starts and lengths,
the trimmed text and quality buffers byte for byte, pads and the 64 spare bytes included, the block table, the longest read,
the layout's size.  No tolerance anywhere.

Geometry the shapes aim at: the find kernel is one wavefront per read, four reads per workgroup, instantiated for 2, 4, 6, 8
and 16 words per plane; a position reads three neighbouring 32-bit words of every plane and shifts them by c mod 32; an adapter
is two words per plane; the quality walk takes 64 bytes a round from the far end; the write kernel is a lane per 64-byte block
of the output; the layout scan is the parse's, in blocks of 1 024 records.  The shapes are the smallest at which these can go
wrong, not a workload."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import merge_pairs_ref as mref  # noqa: E402
import read_overlaps_ref as oref  # noqa: E402
import trim_reads_ref as tref  # noqa: E402

pytestmark = pytest.mark.gpu

AD = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"  # 33 bases: more than one word


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


@pytest.fixture(scope="module")
def searchers(sassy):
    return {"dna": sassy.Searcher("dna", rc=False), "iupac": sassy.Searcher("iupac", rc=False)}


def random_seq(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), n).astype(np.uint8)) if n else b""


def random_qual(rng, n, lo=33, hi=75):
    return bytes(rng.integers(lo, hi, n).astype(np.uint8))


def with_quals(rng, seqs):
    return [(s, random_qual(rng, len(s))) for s in seqs]


def compare(trimmed, records, want, ctx, kept=True):
    """a trimmed handle and the call's records against (records, sequences, qualities) of the helper: everything the handle holds"""
    want_records, seqs, quals = want
    starts, lens, text = mref.layout_of(seqs)
    assert len(trimmed) == len(seqs), (ctx, len(trimmed), len(seqs))
    if records is not None:
        bad = np.flatnonzero(records != want_records)
        assert records.dtype == want_records.dtype and not bad.size, (ctx, "record", bad[:1], records[bad[:1]], want_records[bad[:1]])
    q0 = starts if kept else 0 * starts
    q1 = lens if kept else 0 * lens
    for name, got, exp in (("seq_start", trimmed.seq_starts, starts), ("seq_len", trimmed.seq_lens, lens), ("qual_start", trimmed.qual_starts, q0),
                           ("qual_len", trimmed.qual_lens, q1), ("id_start", trimmed.id_starts, 0 * lens), ("id_len", trimmed.id_lens, 0 * lens)):
        bad = np.flatnonzero(got != exp)
        assert not bad.size, (ctx, name, "read", int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
    assert trimmed.longest == (int(lens.max()) if len(lens) else 0) and trimmed.text_bytes == text.size and trimmed.ptr, ctx
    assert bool(trimmed.qual_ptr) == kept, ctx
    buffers = [("text", trimmed.download_text(), text)]
    if kept:
        buffers.append(("quality", trimmed.download_quality_text(), mref.layout_of(quals)[2]))
    for what, got, exp in buffers:
        got = np.frombuffer(got, dtype=np.uint8)
        diff = np.flatnonzero(got != exp)
        if diff.size:
            at = int(diff[0])
            read = int(np.searchsorted(starts, at, side="right")) - 1
            pytest.fail(f"{ctx}: {what}: first differing byte {at} of {exp.size} (block {at // 64}), read {read}, column {at - int(starts[read])} of "
                        f"{int(lens[read])}, record {want_records[read].tolist()}: got {int(got[at])}, want {int(exp[at])}")
    assert np.array_equal(trimmed.download_rem(), mref.rem_of(starts, lens)), (ctx, "rem")


def launches(profile, reads):
    """stats.scan_launches counts the kernels run: none without a read; else the find kernel, the three kernels of the layout
    scan and the write kernel, and in front of them the Dna look where a dna searcher's batch has a block to look at"""
    if not reads:
        return 0
    return 5 + (profile == "dna" and any(len(r[0] if isinstance(r, tuple) else r) for r in reads))


def check(searchers, profile, reads, adapters, ctx, W=None, **kw):
    """the call over a list of (sequence, quality) or of sequences against the helper"""
    s = searchers[profile]
    trimmed, records = s.trim_reads(reads, adapters, with_records=True, **kw)
    want = tref.expected_trim(profile, reads, adapters, **kw)
    try:
        compare(trimmed, records, want, (ctx, profile, kw), kept=bool(reads) and isinstance(reads[0], tuple))
        st = s.stats()
        assert st["scan_launches"] == launches(profile, reads) and st["candidates"] == int((want[0]["adapter"] >= 0).sum()), (ctx, st)
        if W is not None:
            assert st["word_rows"] == W, (ctx, st["word_rows"], W)
    finally:
        trimmed.free()
    return want


# ================================================================ the definition's own cases
def test_the_cases_written_out_by_hand(searchers):
    for case in tref.HAND:
        for profile in ("dna", "iupac"):
            trimmed, records = searchers[profile].trim_reads([(case["seq"], case["qual"])], case["adapters"], with_records=True, **case["call"])
            assert tuple(records[0].tolist()) == case["record"], (case["name"], profile, records)
            n = case["record"][0]
            assert trimmed.download(0) == case["seq"][:n] and trimmed.quality(0) == case["qual"][:n], (case["name"], profile)
            trimmed.free()
    reads = [(c["seq"], c["qual"]) for c in tref.HAND if c["adapters"] == [tref._AD]]
    check(searchers, "dna", reads, [tref._AD], "the hand cases of one adapter as a batch", min_length=6)


# ================================================================ positions
@pytest.mark.parametrize("la,W", [(70, 4), (130, 6)])
def test_an_adapter_at_every_position(searchers, la, W):
    """The adapter planted at every position of a read: across the 32- and 64-bit word borders, and off the read's end at every
    prefix length 1 .. m."""
    rng = np.random.default_rng(la)
    reads = []
    for c in range(la):
        s = bytearray(random_seq(rng, la))
        s[c:] = (AD + bytes(s[c:]))[:la - c]
        reads.append(bytes(s))
    for profile in ("dna", "iupac"):
        want = check(searchers, profile, with_quals(rng, reads), [AD], ("every position", la), W=W, min_overlap=1, max_permille=0)
        assert (want[0]["adapter_pos"] <= np.arange(la)).all() and (want[0]["adapter_pos"][:la - 3] == np.arange(la - 3)).sum() >= la - 10
        check(searchers, profile, reads, [AD], ("every position, one substitution allowed, no qualities", la), W=W, min_overlap=5, k=1, max_permille=100)


@pytest.mark.parametrize("longest,W", [(64, 2), (128, 4), (192, 6), (256, 8), (512, 16)])
def test_one_batch_per_instantiation(searchers, longest, W):
    rng = np.random.default_rng(W)
    lens = [longest, 0, 1, longest - 1, longest // 2 + 1, 33, longest]
    reads = []
    for i, n in enumerate(lens):
        s = bytearray(random_seq(rng, n))
        if n > 40 and i % 2 == 0:
            c = n - int(rng.integers(1, 40))
            s[c:] = (AD + bytes(s[c:]))[:n - c]
        reads.append((bytes(s), bytes(np.clip(70 - np.arange(n) * 40 // max(n, 1) + rng.integers(-6, 7, n), 33, 126).astype(np.uint8))))
    for profile in ("dna", "iupac"):
        check(searchers, profile, reads, [AD, AD[:12]], ("instance", longest), W=W, quality_cutoff=25, min_length=10)
        check(searchers, profile, reads, [AD], ("instance, no cutoff", longest), W=W)
    # just over the instance's limit takes the next one
    if longest < 512:
        check(searchers, "dna", [(random_seq(rng, longest + 1), random_qual(rng, longest + 1))], [AD], ("one over", longest),
              W={64: 4, 128: 6, 192: 8, 256: 16}[longest])


def test_read_lengths_around_min_overlap_and_the_block(searchers):
    rng = np.random.default_rng(3)
    mo = 5
    for lens in ([0, 1, mo - 1, mo, 63, 64, 65], [65, 64, 63, mo, mo - 1, 1, 0], [0, 0], [mo]):
        reads = []
        for n in lens:
            reads.append((AD[:n] if n <= mo else random_seq(rng, n - mo) + AD[:mo], random_qual(rng, n)))
        for profile in ("dna", "iupac"):
            want = check(searchers, profile, reads, [AD], ("lengths", lens), min_overlap=mo, max_permille=0)
            assert [int(a) for a in want[0]["adapter"]] == [0 if n >= mo else -1 for n in lens]


# ================================================================ adapters
def test_ties_at_every_level_of_the_order(searchers):
    body = b"CCTTGGAACCTTGGAACCTT"
    a13 = AD[:13]
    cases = [
        # level 1, the smallest c: an adapter with one mismatch further left beats a perfect one further right
        (body + b"AGATCGGTAGAGC" + b"GG" + a13, [a13], dict(k=1, max_permille=100), (20, 0, 13, 1)),
        # level 2, the density at one c: 0 / 8 beats 1 / 13
        (body + b"AGATCGGTAGAGC", [a13, b"AGATCGGT"], dict(k=1, max_permille=100), (20, 1, 8, 0)),
        # level 3, the overlap at equal density: 13 rows beat 8
        (body + a13, [a13[:8], a13], dict(), (20, 1, 13, 0)),
        # level 4, the smaller j
        (body + a13, [b"TTTTTTTT", a13, a13], dict(), (20, 1, 13, 0)),
        # ... and off the end, where both overlaps are cut to the same rows
        (body + a13[:6], [a13[:8], a13], dict(), (20, 0, 6, 0)),
    ]
    for seq, adapters, kw, (c, j, ov, mm) in cases:
        for profile in ("dna", "iupac"):
            want = check(searchers, profile, [(seq, b"I" * len(seq))], adapters, ("tie", adapters), **kw)
            r = want[0][0]
            assert (int(r["adapter_pos"]), int(r["adapter"]), int(r["overlap"]), int(r["mismatches"])) == (c, j, ov, mm), (adapters, r)


def test_sixty_four_adapters_and_adapters_of_one_and_sixty_four_bytes(sassy, searchers):
    rng = np.random.default_rng(64)
    adapters = [random_seq(rng, int(rng.integers(8, 65))) for _ in range(64)]
    adapters[63], adapters[17] = random_seq(rng, 64), random_seq(rng, 64)
    reads = []
    for i in range(96):
        n = int(rng.integers(40, 190))
        s = bytearray(random_seq(rng, n))
        if i % 4:
            ad, c = adapters[(i * 7) % 64], int(rng.integers(0, n))
            s[c:] = (ad + bytes(s[c:]))[:n - c]
        reads.append(bytes(s))
    for profile in ("dna", "iupac"):
        want = check(searchers, profile, with_quals(rng, reads), adapters, "64 adapters", W=6, min_overlap=8, k=2)
        assert len(set(want[0]["adapter"].tolist())) > 30 and 63 in want[0]["adapter"]
    # one byte: the first G of every read; 64 bytes whole and as a prefix
    check(searchers, "dna", with_quals(rng, reads[:9]), [b"G"], "an adapter of one byte", min_overlap=1)
    long_ = adapters[63]
    reads = [random_seq(rng, 30) + long_ + random_seq(rng, 10), random_seq(rng, 100) + long_, random_seq(rng, 95) + long_[:63], long_, long_[:1]]
    check(searchers, "iupac", with_quals(rng, reads), [long_], "an adapter of 64 bytes", min_overlap=1, max_permille=0)
    with pytest.raises(sassy.SassyHipError, match="at most 64 adapters"):
        searchers["dna"].trim_reads(reads, adapters + [b"ACGT"])


# ================================================================ parameters
def test_k_and_max_permille_at_their_borders(searchers):
    body = b"CCTTGGAACCTTGGAACCTT"
    twenty = AD[:20]
    two = bytearray(twenty)
    two[3], two[11] = ord("C"), ord("C")   # AGATCGG... -> two mismatches in 20 rows: 100 permille exactly
    three = bytearray(two)
    three[17] = ord("T") if three[17] != ord("T") else ord("A")
    reads = [(body + twenty, None), (body + bytes(two), None), (body + bytes(three), None)]
    reads = [(s, b"I" * len(s)) for s, _ in reads]
    for profile in ("dna", "iupac"):
        for kw, found in ((dict(k=0), [1, 0, 0]), (dict(k=2), [1, 1, 0]), (dict(k=3, max_permille=100), [1, 1, 0]), (dict(k=3, max_permille=150), [1, 1, 1]),
                          (dict(k=2, max_permille=99), [1, 0, 0]), (dict(max_permille=0), [1, 0, 0]), (dict(k=1 << 40, max_permille=1000), [1, 1, 1])):
            want = check(searchers, profile, reads, [twenty], ("borders", kw), min_overlap=20, **kw)
            assert (want[0]["adapter"] >= 0).astype(int).tolist() == found, (kw, want[0])


def test_iupac_n_in_read_and_adapter(sassy, searchers):
    rng = np.random.default_rng(8)
    body = random_seq(rng, 25)
    ad = b"AGATNGGAAGNGC"
    reads = [body + b"AGATCGGAAGAGC" + b"TT", body + b"AGATTGGAAGTGC", body + b"ANATCGGNAGAGC", body + b"AGATCGGAAGAGX", body + b"NNNN", b"NNNNNNNNNNNNN" + body]
    want = check(searchers, "iupac", with_quals(rng, reads), [ad], "N", min_overlap=4, max_permille=0)
    assert want[0]["adapter_pos"].tolist()[:3] == [25, 25, 25] and want[0]["adapter_pos"][5] == 0
    check(searchers, "iupac", with_quals(rng, reads), [b"RYACGT", ad], "more codes", min_overlap=3, k=1)


# ================================================================ quality and length
def test_quality_walks_across_the_rounds(searchers):
    rng = np.random.default_rng(12)
    reads = []
    for n in (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256):
        s = random_seq(rng, n)
        q = np.full(n, 70, dtype=np.uint8)
        reads.append((s, bytes(q)))                                   # nothing to cut
        for cut in sorted({0, 1, n // 2, max(n - 65, 0), max(n - 64, 0), max(n - 63, 0), n - 1}):
            q = np.full(n, 70, dtype=np.uint8)
            q[cut:] = 35
            reads.append((s, bytes(q)))
            if cut + 3 < n:                                           # a good stretch inside the tail: the stop
                q[cut + 1:cut + 3] = 126
                reads.append((s, bytes(q)))
        reads.append((s, random_qual(rng, n, 33, 60)))
        reads.append((s, bytes(np.clip(75 - np.arange(n) * 45 // n + rng.integers(-8, 9, n), 33, 126).astype(np.uint8))))
    for profile in ("dna", "iupac"):
        want = check(searchers, profile, reads, [], "walks, no adapter", quality_cutoff=20)
        assert len(set(want[0]["quality_len"].tolist())) > 30 and (want[0]["adapter"] == -1).all()
        check(searchers, profile, reads, [AD], "walks, an adapter", quality_cutoff=30, min_length=20)
    check(searchers, "dna", reads, [], "cutoff 93", quality_cutoff=93)
    check(searchers, "dna", reads, [], "cutoff 1", quality_cutoff=1)


def test_the_adapter_is_searched_in_front_of_the_quality_cut(searchers):
    body = b"CCTTGGAACCTTGGAACCTT"
    seq = body + AD[:13] + b"ACGTACGTAC"
    for low_from, (lq, cut, j) in ((43, (43, 20, 0)), (33, (33, 20, 0)), (28, (28, 20, 0)), (22, (22, 22, -1)), (20, (20, 20, -1))):
        qual = b"I" * low_from + b"#" * (len(seq) - low_from)
        want = check(searchers, "dna", [(seq, qual)], [AD[:13]], ("quality then adapter", low_from), quality_cutoff=20, min_overlap=3)
        r = want[0][0]
        assert (int(r["quality_len"]), int(r["adapter_pos"]), int(r["adapter"])) == (lq, cut, j), (low_from, r)


def test_min_length_drops_first_last_all_and_alternate_reads(searchers):
    rng = np.random.default_rng(4)
    short, long_ = random_seq(rng, 12) + AD, random_seq(rng, 70) + AD
    for order in ([short, long_, long_], [long_, long_, short], [short] * 3, [short, long_] * 3, [long_, short] * 3, [long_] * 2):
        want = check(searchers, "dna", with_quals(rng, order), [AD], ("min_length", [len(x) for x in order]), min_length=13)
        assert [int(n) for n in want[0]["length"]] == [0 if x is short else 70 for x in order]
        check(searchers, "dna", order, [], ("min_length, nothing else", len(order)), min_length=50)
    # nothing left of any read, and no read at all: the 64 spare bytes alone
    for reads in ([short] * 3, [b"", b""], []):
        trimmed = searchers["dna"].trim_reads(with_quals(rng, reads), [AD], min_length=13)
        assert len(trimmed) == len(reads) and trimmed.text_bytes == 64 and trimmed.download_text() == bytes(64)
        assert bool(trimmed.qual_ptr) == bool(reads) and (not reads or trimmed.download_quality_text() == bytes(64))  # (an empty list brings no qualities)
        assert trimmed.longest == 0 and searchers["dna"].stats()["scan_launches"] == launches("dna", reads)
        trimmed.free()


# ================================================================ batch size and input source
def test_more_reads_than_one_block_of_the_scan_and_resident_raw_input(sassy, searchers):
    rng = np.random.default_rng(2049)
    reads = []
    for i in range(2 * 1024 + 37):   # three blocks of the record scan
        n = int(rng.integers(0, 48))
        s = bytearray(random_seq(rng, n))
        if n > 8 and i % 3:
            c = int(rng.integers(0, n))
            s[c:] = (AD + bytes(s[c:]))[:n - c]
        reads.append(bytes(s))
    reads = with_quals(rng, reads)
    want = check(searchers, "dna", reads, [AD], "2 085 reads", W=2, min_overlap=4, quality_cutoff=12, min_length=5)
    assert (want[0]["length"] == 0).sum() > 100 and (want[0]["adapter"] >= 0).sum() > 500
    raw = sassy.fastq_from_sequences([x[0] for x in reads], [x[1] for x in reads])
    buf = sassy.DeviceBuffer((len(raw) + 63) // 64 * 64)
    buf.upload(raw)
    dev = sassy.DeviceReads(sassy.DeviceText(buf.ptr, len(raw), owner=buf), keep_quality=True)
    plain = sassy.DeviceReads(raw)
    try:
        state = lambda h: (h.download_text(), h.download_rem().tolist(), h.seq_starts.tolist(), h.seq_lens.tolist())  # noqa: E731
        before = state(dev), dev.download_quality_text()
        trimmed, records = searchers["dna"].trim_reads(dev, [AD], 4, quality_cutoff=12, min_length=5, with_records=True)
        compare(trimmed, records, want, "resident raw input")
        trimmed.free()
        assert (state(dev), dev.download_quality_text()) == before   # the input is only read
        # without kept qualities: the same cuts where no cutoff is asked, and a handle without a quality buffer
        trimmed, records = searchers["dna"].trim_reads(plain, [AD], 4, min_length=5, with_records=True)
        compare(trimmed, records, tref.expected_trim("dna", [x[0] for x in reads], [AD], 4, min_length=5), "qualities not kept", kept=False)
        trimmed.free()
    finally:
        for h in (dev, plain, buf):
            h.free()


# ================================================================ chaining
@pytest.fixture(scope="module")
def batch():
    """80 reads of 30 .. 200 bases, most with an adapter somewhere, some dropped; the helper's result, once."""
    rng = np.random.default_rng(31)
    reads = []
    for i in range(80):
        n = int(rng.integers(30, 200))
        s = bytearray(random_seq(rng, n))
        if i % 5:
            c = int(rng.integers(5, n))
            s[c:] = (AD + bytes(s[c:]))[:n - c]
        reads.append(bytes(s))
    reads = with_quals(rng, reads)
    call = dict(min_overlap=4, k=2, max_permille=100, quality_cutoff=0, min_length=20)
    return reads, call, tref.expected_trim("dna", reads, [AD], **call)


def test_the_batch_calls_take_the_trimmed_handle(sassy, searchers, batch):
    reads, call, (want_records, seqs, quals) = batch
    trimmed = searchers["dna"].trim_reads(reads, [AD], **call)
    try:
        assert sum(1 for x in seqs if not x) >= 3 and sum(1 for x in seqs if x) >= 60
        pats = [seqs[1][5:17], next(x for x in seqs if len(x) > 40)[20:32], oref.revcomp("dna", seqs[2][-12:]), b"ACGTACGTACGT"]
        host, dev = sassy.Searcher("dna", rc=True), sassy.Searcher("dna", rc=True)
        key = lambda m: (m.pattern_idx, m.text_idx, m.text_start, m.text_end, m.cost, m.strand, m.cigar)  # noqa: E731
        for fn in (lambda x, t: [a.tolist() for a in x.hamming_best_pattern(pats, t, 2)],
                   lambda x, t: [key(m) for m in x.best_matches(pats, t, 2)],
                   lambda x, t: [key(m) for m in x.search_many(pats, t, 2)]):
            a, b = fn(host, seqs), fn(dev, trimmed)
            assert a == b and len(a) > 0
        compare(trimmed, None, (want_records, seqs, quals), "after the batch calls")  # the handle is only read
        # a second trim of the trimmed handle, with a cutoff: its qualities are its own
        again, records = searchers["dna"].trim_reads(trimmed, [b"ACGTACG"], 5, quality_cutoff=15, min_length=10, with_records=True)
        compare(again, records, tref.expected_trim("dna", list(zip(seqs, quals)), [b"ACGTACG"], 5, quality_cutoff=15, min_length=10), "a second trim")
        again.free()
    finally:
        trimmed.free()


def test_two_trimmed_handles_through_merge_pairs(searchers):
    rng = np.random.default_rng(77)
    ad2 = b"CTGTCTCTTATACACATCT"
    r1s, r2s = [], []
    for i in range(40):
        insert = random_seq(rng, int(rng.integers(40, 140)))
        n = 100
        r1 = (insert + AD + random_seq(rng, n))[:n]
        r2 = (oref.revcomp("dna", insert) + ad2 + random_seq(rng, n))[:n]
        r1s.append(r1)
        r2s.append(r2)
    p1, p2 = with_quals(rng, r1s), with_quals(rng, r2s)
    s = searchers["dna"]
    t1, t2 = s.trim_reads(p1, [AD], 5), s.trim_reads(p2, [ad2], 5)
    try:
        w1, w2 = tref.expected_trim("dna", p1, [AD], 5), tref.expected_trim("dna", p2, [ad2], 5)
        compare(t1, None, w1, "r1 trimmed")
        merged, records = s.merge_pairs(t1, t2, 10, 5, 100, with_overlaps=True)
        want = mref.expected_merge("dna", list(zip(w1[1], w1[2])), list(zip(w2[1], w2[2])), 10, 5, 100)
        assert np.array_equal(records, want[0]) and (want[0]["n_accepted"] > 0).sum() > 30
        assert [merged.download(i) for i in range(len(merged))] == want[1] and [merged.quality(i) for i in range(len(merged))] == want[2]
        assert merged.download_text() == mref.layout_of(want[1])[2].tobytes() and merged.download_quality_text() == mref.layout_of(want[2])[2].tobytes()
        merged.free()
    finally:
        t1.free(), t2.free()


# ================================================================ the window call
def test_slice_at_every_begin_mod_16_and_lengths_around_the_block(sassy):
    rng = np.random.default_rng(16)
    widths = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129]
    seqs, begins, lens = [], [], []
    for b in range(0, 34):
        w = widths[b % len(widths)]
        tail = int(rng.integers(0, 7))
        seqs.append(random_seq(rng, b + w + tail, b"ACGTN"))
        begins.append(b)
        lens.append(w)
    for b, w in ((63, 64), (64, 64), (65, 63), (0, 200), (129, 1)):
        seqs.append(random_seq(rng, b + w))
        begins.append(b)
        lens.append(w)
    quals = [random_qual(rng, len(s), 33, 127) for s in seqs]
    for kept in (True, False):
        h = sassy.DeviceReads.from_sequences(seqs, quals if kept else None)
        try:
            before = h.download_text()
            cut = h.slice(begins, lens)
            want_s = [s[b:b + w] for s, b, w in zip(seqs, begins, lens)]
            want_q = [q[b:b + w] for q, b, w in zip(quals, begins, lens)]
            compare(cut, None, (np.zeros(len(seqs), dtype=tref.DTYPE), want_s, want_q), ("slice", kept), kept=kept)
            cut.free()
            # one number for all: a leading UMI of 8 bases split off and the rest
            ok = [i for i, s in enumerate(seqs) if len(s) >= 8]
            sub = sassy.DeviceReads.from_sequences([seqs[i] for i in ok], [quals[i] for i in ok] if kept else None)
            umi, rest = sub.slice(0, 8), sub.slice(8, [len(seqs[i]) - 8 for i in ok])
            assert [umi.download(i) for i in range(len(ok))] == [seqs[i][:8] for i in ok]
            assert [rest.download(i) for i in range(len(ok))] == [seqs[i][8:] for i in ok]
            if kept:
                assert [rest.quality(i) for i in range(len(ok))] == [quals[i][8:] for i in ok]
            for x in (umi, rest, sub):
                x.free()
            assert h.download_text() == before
            with pytest.raises(sassy.SassyHipError, match=r"window 2 \[2, \+\d+\) reaches outside its read"):
                h.slice(begins, [w + (40 if i == 2 else 0) for i, w in enumerate(lens)])
        finally:
            h.free()
    empty = sassy.DeviceReads(b"", keep_quality=True)
    cut = empty.slice([], [])
    assert len(cut) == 0 and cut.text_bytes == 64 and cut.download_quality_text() == bytes(64)
    cut.free(), empty.free()


# ================================================================ refusals
def test_refusals_that_read_the_handle(sassy, searchers):
    import ctypes as C
    L = sassy.lib()
    s = searchers["dna"]
    kept = sassy.DeviceReads.from_sequences([b"ACGTACGTACGT"] * 2, [b"IIIIIIIIIIII"] * 2)
    plain = sassy.DeviceReads.from_sequences([b"ACGTACGTACGT"] * 2)
    long_ = sassy.DeviceReads.from_sequences([b"A" * 513, b"ACGT"], [b"I" * 513, b"IIII"])
    other = sassy.DeviceReads.from_sequences([b"ACGTACGTACGN"] * 2, [b"IIIIIIIIIIII"] * 2)

    def refused(searcher, reads, code, word, adapter=b"ACGTAC", cutoff=0, null_out=False):
        out = C.c_void_p(7)
        ptrs, lens = (C.c_char_p * 1)(adapter), (C.c_size_t * 1)(len(adapter))
        rc = L.sassy_hip_trim_reads(searcher._h, reads._handle(), ptrs, lens, 1, 3, 512, 100, cutoff, 0, 0, None, None if null_out else C.byref(out))
        msg = L.sassy_hip_last_error().decode()
        assert rc == code and word in msg and (null_out or out.value is None), (rc, msg, word, out.value)

    try:
        refused(s, long_, -1, "at most 512 bytes")
        refused(s, plain, -1, "parsed without SASSY_HIP_KEEP_QUALITY", cutoff=20)
        refused(s, long_, -1, "at most 512 bytes", cutoff=20, null_out=True)          # the order: the length, the qualities, the pointer
        refused(s, plain, -1, "SASSY_HIP_KEEP_QUALITY", cutoff=20, null_out=True)
        refused(s, kept, -1, "must not be null (out_trimmed)", null_out=True)
        refused(s, other, -1, "the reads hold other bytes than A, C, G, T")
        refused(s, kept, -1, "adapter 0 holds other bytes than A, C, G, T", adapter=b"ACGTNC")
        refused(sassy.Searcher("ascii", rc=False), kept, -1, "use a dna or an iupac searcher")
        with pytest.raises(sassy.SassyHipError, match="KEEP_QUALITY"):
            s.trim_reads(plain, [b"ACGTAC"], quality_cutoff=20)
        # an adapter with another letter is refused under dna whatever the batch holds, an empty one included
        none = sassy.DeviceReads(b"", keep_quality=True)
        refused(s, none, -1, "adapter 0 holds other bytes than A, C, G, T", adapter=b"ACGTNC")
        none.free()
        # searches in flight: a ticket is open on the searcher (the last refusal of the order: everything else is right)
        text = b"ACGT" * 64
        buf = sassy.DeviceBuffer(len(text) + 256)
        buf.upload(text)
        busy = sassy.Searcher("dna", rc=False)
        ticket = busy.search_shard_begin(b"ACGTACGTACGT", buf.ptr, 0, len(text), 0, len(text), 1)
        try:
            refused(busy, kept, -1, "searches are in flight on this searcher")
            refused(busy, long_, -1, "at most 512 bytes")                                # ... and everything else comes first
            refused(busy, kept, -1, "must not be null (out_trimmed)", null_out=True)
        finally:
            assert len(busy.search_finish(ticket)) > 0
        trimmed = busy.trim_reads(kept, [b"ACGTAC"])                                     # the ticket finished: the call is taken
        assert len(trimmed) == 2
        trimmed.free(), buf.free()
        # and the call still works afterwards, under iupac with the N as well, and without qualities where none are asked for
        for searcher, reads in ((searchers["iupac"], other), (s, kept), (s, plain)):
            trimmed = searcher.trim_reads(reads, [b"ACGTNC" if searcher is searchers["iupac"] else b"ACGTAC"])
            assert len(trimmed) == 2 and bool(trimmed.qual_ptr) == (reads is not plain)
            trimmed.free()
    finally:
        for h in (kept, plain, long_, other):
            h.free()
    with pytest.raises(sassy.SassyHipError, match="freed"):
        s.trim_reads(kept, [b"ACGTAC"])


# ================================================================ the CLI
def test_cli_trim_writes_the_helpers_reads_and_rows(sassy, batch, tmp_path, monkeypatch, capsysbinary):
    from sassy_amd import cli
    reads, call, (want_records, seqs, quals) = batch
    raw = [b"@read%d x\r\n%s\r\n+read%d\r\n%s\r\n" % (i, s, i, q) for i, (s, q) in enumerate(reads)]
    f = tmp_path / "in.fq"
    f.write_bytes(b"".join(raw))
    ids = ["read%d x" % i for i in range(len(reads))]
    want = b"".join(b"@" + i.encode() + b"\n" + s + b"\n+\n" + q + b"\n" for i, s, q in zip(ids, seqs, quals) if s)
    out = tmp_path / "t.fq"
    for batch_bytes in (cli.BATCH_BYTES, 3000):  # (the second: many chunks)
        monkeypatch.setattr(cli, "BATCH_BYTES", batch_bytes)
        argv = ["trim", str(f), "-a", AD.decode(), "--min-overlap", "4", "-k", "2", "--max-permille", "100", "-m", "20"]
        assert cli.main(argv + ["-o", str(out), "--tsv"]) == 0
        assert out.read_bytes() == want
        assert (tmp_path / "t.fq.tsv").read_text() == cli.TRIM_HEADER + "".join(cli.trim_rows(ids, want_records))
        capsysbinary.readouterr()
        assert cli.main(argv) == 0
        assert capsysbinary.readouterr().out == want
    # quality only
    assert cli.main(["trim", str(f), "-q", "25", "-o", str(out)]) == 0
    w = tref.expected_trim("dna", reads, [], quality_cutoff=25)
    assert out.read_bytes() == b"".join(b"@" + i.encode() + b"\n" + s + b"\n+\n" + q + b"\n" for i, s, q in zip(ids, w[1], w[2]) if s)
