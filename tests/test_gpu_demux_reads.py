"""Demultiplexing on the device (sassy_amd/csrc/demux_reads.hip) and the gather against their definition
(tests/helpers/demux_reads_ref.py): every comparison is exact equality -- the records, the order, the bounds, the starts and
lengths, the text and quality buffers byte for byte, pads and the 64 spare bytes included, the block table, the longest read, the
layout's size, the stats.  No tolerance anywhere.

Geometry the shapes aim at: the assign kernel is a lane per read in workgroups of 256; a window is up to 64 bytes at any alignment,
fetched as five 16-byte pieces; the sort's key has as many bits as B has; the bounds kernel is a lane per label; the write kernel
is a lane per 64-byte block of the output with a source table; the layout scan is the parse's, in blocks of 1 024 records.  The
shapes are the smallest at which these can go wrong, not a workload."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import demux_reads_ref as dref  # noqa: E402
import trim_reads_ref as tref  # noqa: E402

pytestmark = pytest.mark.gpu

MIXED_BARCODES = [b"ACGTACGT", b"ACGTACAA", b"TTGGCCAA", b"GGATTCCA"]  # tests/test_demux_reads_cpu.py checks the groups of this batch
MIXED_SEED = 1
ATS = list(range(16)) + [63, 64, 127, 128, 447, 448]


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


def with_quals(rng, seqs):
    return [(s, bytes(rng.integers(33, 75, len(s)).astype(np.uint8))) for s in seqs]


def compare_handle(reads, seqs, quals, ctx):
    """a handle against the sequences (and qualities, or None) it must hold: everything the handle holds"""
    kept = quals is not None
    text, qual, starts, rem, longest = dref.layout(seqs, quals)
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    assert len(reads) == len(seqs), (ctx, len(reads), len(seqs))
    zero = 0 * lens
    for name, got, exp in (("seq_start", reads.seq_starts, starts), ("seq_len", reads.seq_lens, lens), ("qual_start", reads.qual_starts, starts if kept else zero),
                           ("qual_len", reads.qual_lens, lens if kept else zero), ("id_start", reads.id_starts, zero), ("id_len", reads.id_lens, zero)):
        bad = np.flatnonzero(got != exp)
        assert not bad.size, (ctx, name, "record", int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
    assert reads.longest == longest and reads.text_bytes == len(text) and reads.ptr and bool(reads.qual_ptr) == kept, (ctx, reads.longest, reads.text_bytes)
    buffers = [("text", reads.download_text(), text)]
    if kept:
        buffers.append(("quality", reads.download_quality_text(), qual))
    for what, got, exp in buffers:
        if got != exp:
            a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(exp, dtype=np.uint8)
            at = int(np.flatnonzero(a != b)[0])
            rec = int(np.searchsorted(starts, at, side="right")) - 1
            pytest.fail(f"{ctx}: {what}: first differing byte {at} of {len(exp)} (block {at // 64}), record {rec}, column {at - int(starts[rec])} of "
                        f"{int(lens[rec])}: got {int(a[at])}, want {int(b[at])}")
    assert np.array_equal(reads.download_rem(), rem), (ctx, "rem")


def launches(profile, reads):
    """stats.scan_launches: none without a read; else the assign kernel, the sort, bounds, place, the three kernels of the layout
    scan and the write kernel, and in front of them the Dna look where a dna searcher's batch has a block to look at"""
    if not reads:
        return 0
    return 8 + (profile == "dna" and any(len(r[0] if isinstance(r, tuple) else r) for r in reads))


def check(sassy, searchers, profile, reads, barcodes, ctx, **kw):
    """the call over a list of (sequence, quality) or of sequences against the helper; returns the helper's result"""
    s = searchers[profile]
    want = dref.expected_demux(profile, reads, barcodes, **kw)
    d = sassy.demux_reads(s, reads, barcodes, with_records=True, **kw)
    try:
        records, order, bounds, seqs, quals = want
        bad = np.flatnonzero(d.records != records)
        assert d.records.dtype == records.dtype and not bad.size, (ctx, "record", bad[:1], d.records[bad[:1]], records[bad[:1]])
        assert np.array_equal(d.order, order) and d.order.dtype == np.uint64, (ctx, "order")
        assert np.array_equal(d.bounds, bounds) and d.bounds.dtype == np.uint64, (ctx, "bounds", d.bounds, bounds)
        assert np.array_equal(d.counts, np.diff(bounds.astype(np.int64))) and d.n_samples == len(barcodes)
        kept = bool(reads) and isinstance(reads[0], tuple)
        compare_handle(d.reads, seqs, quals if kept else None, (ctx, profile, kw))
        st = s.stats()
        assert st["scan_launches"] == launches(profile, reads) and st["candidates"] == int((records["sample"] >= 0).sum()), (ctx, st)
    finally:
        d.free()
    return want


# ================================================================ the definition's own cases
def test_the_cases_written_out_by_hand(sassy, searchers):
    for case in dref.HAND:
        for profile in ("dna", "iupac"):
            d = sassy.demux_reads(searchers[profile], [case["seq"]], case["barcodes"], with_records=True, **case["call"])
            assert tuple(d.records[0].tolist()) == case["record"] + (0,), (case["name"], profile, d.records)
            assert d.reads.download(0) == case["kept"] and d.order.tolist() == [0], (case["name"], profile)
            d.free()
    three = [c for c in dref.HAND if len(c["barcodes"]) == 3 and c["call"] == dref.HAND[0]["call"]]
    check(sassy, searchers, "dna", [c["seq"] for c in three], three[0]["barcodes"], "hand cases as a batch", **three[0]["call"])


# ================================================================ the read count: the wavefront, the workgroup, the scan's blocks
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_the_seeded_mixed_batch_at_every_read_count(sassy, searchers, n):
    reads = dref.mixed_batch(n, MIXED_SEED, MIXED_BARCODES)
    want = check(sassy, searchers, "dna", reads, MIXED_BARCODES, ("mixed", n), k=1, min_delta=1)
    if n >= 63:  # non-trivial by the helper alone: every group holds at least a tenth of the reads
        g = dref.groups(want[0], 1)
        assert all(v * 10 >= n for v in g.values()), g
    if n == 0:
        assert want[2].tolist() == [0] * (len(MIXED_BARCODES) + 2)


@pytest.mark.parametrize("end3,clip,at", [(True, True, 0), (True, False, 3), (True, True, 5), (False, False, 0), (False, True, 7)])
def test_both_ends_with_and_without_clip(sassy, searchers, end3, clip, at):
    for profile in ("dna", "iupac"):
        reads = dref.mixed_batch(333, 4, MIXED_BARCODES, at=at, end3=end3)
        want = check(sassy, searchers, profile, reads, MIXED_BARCODES, ("ends", end3, clip, at), k=1, min_delta=1, at=at, end3=end3, clip=clip)
        assert all(v * 10 >= 333 for v in dref.groups(want[0], 1).values())


# ================================================================ the barcode count: the radix key's width
@pytest.mark.parametrize("B,profile", [(1, "dna"), (255, "dna"), (256, "iupac"), (4096, "iupac"), (4096, "dna")])
def test_barcode_counts_around_the_key_widths(sassy, searchers, B, profile):
    rng = np.random.default_rng(B)
    m = 8
    codes = rng.choice(4 ** m, size=B, replace=False)
    barcodes = [bytes(b"ACGT"[(int(c) >> (2 * i)) & 3] for i in range(m)) for c in codes]
    if profile == "iupac":  # wildcards on the pattern side, and the last barcode a near twin of the first
        barcodes = [b[:3] + b"N" + b[4:] if j % 7 == 3 else b for j, b in enumerate(barcodes)]
    reads = []
    for r in range(300):
        j = (B - 1 - r // 2) % B if r % 2 else int(rng.integers(B))     # the highest labels are used
        w = bytearray(barcodes[j].replace(b"N", b"A"))
        if r % 5 == 0:
            w[int(rng.integers(m))] = b"ACGT"[int(rng.integers(4))]
        reads.append(bytes(w) + random_seq(rng, int(rng.integers(0, 80))))
    reads += [b"", b"ACG"]
    want = check(sassy, searchers, profile, with_quals(rng, reads), barcodes, ("B", B), k=1, min_delta=1)
    labels = want[0]["sample"]
    assert (labels >= 0).sum() > 100 and (B == 1 or labels.max() == B - 1)


def test_every_read_to_one_sample_every_read_unassigned_and_empty_samples_between_full_ones(sassy, searchers):
    rng = np.random.default_rng(3)
    bcs = [b"AAAAAA", b"CCCCCC", b"GGGGGG", b"TTTTTT", b"ACACAC"]
    tails = [random_seq(rng, int(rng.integers(0, 130))) for _ in range(200)]
    one = check(sassy, searchers, "dna", with_quals(rng, [bcs[2] + t for t in tails]), bcs, "one sample", k=0)
    assert one[2].tolist() == [0, 0, 0, 200, 200, 200, 200]
    none = check(sassy, searchers, "dna", with_quals(rng, [b"GTGTGT" + t for t in tails]), bcs, "all unassigned", k=1)
    assert none[2].tolist() == [0, 0, 0, 0, 0, 0, 200] and none[1].tolist() == list(range(200))
    gaps = check(sassy, searchers, "iupac", with_quals(rng, [bcs[(i % 2) * 3 + 1] + t for i, t in enumerate(tails)]), bcs, "samples 1 and 4", k=0)
    assert gaps[2].tolist() == [0, 0, 100, 100, 100, 200, 200]


def test_a_clip_that_leaves_nothing(sassy, searchers):
    reads = [(b"GG" + MIXED_BARCODES[i % 4], b"I" * 10) for i in range(70)]
    want = check(sassy, searchers, "dna", reads, MIXED_BARCODES, "la = at + m", k=0, min_delta=1, at=2)
    assert (want[0]["sample"] >= 0).all() and all(s == b"" for s in want[3])
    d = sassy.demux_reads(searchers["dna"], reads, MIXED_BARCODES, k=0, at=2)
    assert d.reads.text_bytes == 64 and d.reads.download_text() == bytes(64) and int(d.reads.seq_lens.sum()) == 0
    kept, idx = d.reads.nonempty()
    assert len(kept) == 0 and len(idx) == 0 and kept.text_bytes == 64
    kept.free()
    d.free()


# ================================================================ the window: every residue, across the 64-byte boundaries
@pytest.mark.parametrize("m", [1, 8, 31, 32, 33, 63, 64])
def test_the_window_at_every_alignment(sassy, searchers, m):
    """As tests/c/demux_step_driver.cc: `at` at every residue mod 16 and at and across 64, 128 and 448; reads of at + m - 1 (no
    window), at + m (the clip leaves nothing), at + m + 1, 0 and 512 bytes; both ends, both profiles."""
    rng = np.random.default_rng(m)
    letters = {"dna": b"ACGT", "iupac": b"ACGTNRYKMSWBDHVacgtn"}
    for profile in ("dna", "iupac"):
        bcs = [random_seq(rng, m, letters[profile]) for _ in range(3)]
        bcs[1] = bcs[0][:m // 2] + random_seq(rng, 1, letters[profile]) + bcs[0][m // 2 + 1:]
        for at in ATS:
            if at + m > 512:
                continue
            for end3 in (False, True):
                reads = []
                for la in (at + m - 1, at + m, at + m + 1, 0, 512):
                    if la > 512:
                        continue
                    s = bytearray(random_seq(rng, la, letters[profile]))
                    if la >= at + m:
                        w = la - at - m if end3 else at
                        s[w:w + m] = bcs[int(rng.integers(3))]
                        if m > 1 and rng.integers(2):
                            s[w + int(rng.integers(m))] = letters[profile][int(rng.integers(4))]
                    reads.append(bytes(s))
                check(sassy, searchers, profile, with_quals(rng, reads), bcs, ("window", m, at, end3), k=2, min_delta=int(rng.integers(2)), at=at, end3=end3)


# ================================================================ ties
def test_planted_ties_under_min_delta_0_and_1(sassy, searchers):
    rng = np.random.default_rng(8)
    bcs = [b"ACGTACGT", b"ACGTACAA", b"ACGTACGT", b"TTTTGGGG"]   # 0 and 2 are twins; 1 is two rows from both
    reads = []
    for i in range(130):
        w = [b"ACGTACGT", b"ACGTACGA", b"ACGTACAT", b"TTTTGGGG", b"TTTTGGGC"][i % 5]
        reads.append(w + random_seq(rng, int(rng.integers(0, 70))))
    reads = with_quals(rng, reads)
    zero = check(sassy, searchers, "dna", reads, bcs, "min_delta 0", k=1, min_delta=0)
    one = check(sassy, searchers, "dna", reads, bcs, "min_delta 1", k=1, min_delta=1)
    assert (zero[0]["n_best"] > 1).sum() >= 78 and np.array_equal(zero[0]["n_best"], one[0]["n_best"])
    tied = zero[0]["n_best"] > 1
    assert (zero[0]["sample"][tied] == zero[0]["best"][tied]).all() and (one[0]["sample"][tied] == -1).all()
    assert (zero[0]["sample"] == 2).sum() == 0 and (zero[0]["sample"] == 0).sum() > 50   # the smaller index of the twins
    seven = check(sassy, searchers, "dna", reads, bcs, "min_delta 7", k=1, min_delta=7)   # TTTTGGGG is six rows from ACGTACGT
    assert (one[0]["sample"] >= 0).sum() == 52 and (seven[0]["sample"] >= 0).sum() == 0


# ================================================================ handles
def test_a_handle_without_qualities(sassy, searchers):
    reads = [s for s, _ in dref.mixed_batch(200, 2, MIXED_BARCODES)]
    check(sassy, searchers, "dna", reads, MIXED_BARCODES, "no qualities", k=1)
    check(sassy, searchers, "iupac", reads, MIXED_BARCODES, "no qualities, 3'", k=1, end3=True, clip=False)


def test_the_output_of_a_trim_and_of_a_merge_as_input(sassy, searchers):
    rng = np.random.default_rng(12)
    s = searchers["dna"]
    ad = b"AGATCGGAAGAGC"
    reads = []
    for i, (seq, q) in enumerate(dref.mixed_batch(150, 3, MIXED_BARCODES)):
        seq = seq + (ad + random_seq(rng, 10) if i % 2 else b"")
        reads.append((seq, bytes(rng.integers(33, 75, len(seq)).astype(np.uint8))))
    trimmed = s.trim_reads(reads, [ad], min_overlap=5, k=0)
    _, tseqs, tquals = tref.expected_trim("dna", reads, [ad], min_overlap=5, k=0)
    want = dref.expected_demux("dna", list(zip(tseqs, tquals)), MIXED_BARCODES, k=1)
    d = trimmed.demux(s, MIXED_BARCODES, k=1, with_records=True)
    assert np.array_equal(d.records, want[0]) and np.array_equal(d.order, want[1]) and np.array_equal(d.bounds, want[2])
    compare_handle(d.reads, want[3], want[4], "behind a trim")
    d.free()
    trimmed.free()
    # a merge: R2 is the reverse complement of R1's tail, so every pair merges into R1 itself
    r1 = [(seq, q) for seq, q in dref.mixed_batch(250, 5, MIXED_BARCODES) if len(seq) >= 40]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    r2 = [(seq[-30:].translate(comp)[::-1], q[-30:][::-1]) for seq, q in r1]
    merged = s.merge_pairs(r1, r2, 20, 0, 0)
    mseqs = [merged.download(i) for i in range(len(merged))]
    mquals = [merged.quality(i) for i in range(len(merged))]
    assert sum(1 for a, (b, _) in zip(mseqs, r1) if a == b) > 50   # merged: what the demux sees is a batch of real reads
    want = dref.expected_demux("dna", list(zip(mseqs, mquals)), MIXED_BARCODES, k=1)
    d = merged.demux(s, MIXED_BARCODES, k=1, with_records=True)
    assert np.array_equal(d.records, want[0]) and np.array_equal(d.order, want[1]) and np.array_equal(d.bounds, want[2])
    compare_handle(d.reads, want[3], want[4], "behind a merge")
    d.free()
    merged.free()


# ================================================================ select alone
@pytest.fixture(scope="module")
def batch(sassy):
    rng = np.random.default_rng(21)
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 512] + [int(x) for x in rng.integers(0, 300, 60)]
    reads = with_quals(rng, [random_seq(rng, n, b"ACGTN") for n in lens])
    handle = sassy.DeviceReads.from_sequences([s for s, _ in reads], [q for _, q in reads])
    yield reads, handle
    handle.free()


def check_select(handle, reads, src, ctx, begins=None, lens=None, kept=True):
    want = dref.expected_select(reads, src, begins, lens)
    got = handle.select(src, begins, lens)
    try:
        compare_handle(got, [s for s, _ in want], [q for _, q in want] if kept else None, ctx)
    finally:
        got.free()


def test_select_identity_reversal_repeats_and_nothing(sassy, batch):
    reads, handle = batch
    n = len(reads)
    check_select(handle, reads, list(range(n)), "identity")
    check_select(handle, reads, list(range(n))[::-1], "reversal")
    check_select(handle, reads, [12, 12, 0, 12, 5, 5, 1], "repeats")
    check_select(handle, reads, [], "nothing")
    check_select(handle, reads, [0, 0, 0], "only empty reads")
    rng = np.random.default_rng(2)
    check_select(handle, reads, rng.integers(0, n, 2049).tolist(), "2049 records of 73")
    kept, idx = handle.nonempty()
    assert idx.tolist() == [i for i, (s, _) in enumerate(reads) if s]
    compare_handle(kept, [reads[i][0] for i in idx.tolist()], [reads[i][1] for i in idx.tolist()], "nonempty")
    kept.free()
    plain = sassy.DeviceReads.from_sequences([s for s, _ in reads])
    check_select(plain, [(s, None) for s, _ in reads], [3, 1, 12, 12], "without qualities", kept=False)
    plain.free()


def test_select_shifted_windows_at_every_residue(sassy, batch):
    reads, handle = batch
    rng = np.random.default_rng(4)
    src, begins, lens = [], [], []
    for r, (s, _) in enumerate(reads):
        for b in range(min(len(s), 17) + 1):
            src.append(r)
            begins.append(b)
            lens.append(len(s) - b if b % 2 else int(rng.integers(0, len(s) - b + 1)))
    assert len({b % 16 for b in begins}) == 16 and len(src) > 1024
    check_select(handle, reads, src, "shifted", begins, lens)
    check_select(handle, reads, [12, 11], "one number for all", 3, 100)


def test_select_refusals(sassy, batch):
    reads, handle = batch
    n = len(reads)
    for args, word in ((([n],), f"src 0 = {n} names no read of a batch of {n}"), (([0, 1, 1 << 40],), "src 2 = "),
                       (([12, 1], [0, 1], [512, 1]), "window 1 [1, +1) reaches outside its read of 1 bytes"),
                       (([12], [513], [0]), "window 0 [513, +0) reaches outside its read of 512 bytes"), (([1], [0], None), "given together")):
        with pytest.raises(sassy.SassyHipError) as e:
            handle.select(*args)
        assert word in str(e.value), (word, str(e.value))
    empty = handle.select([])
    with pytest.raises(sassy.SassyHipError) as e:
        empty.select([0])
    assert "names no read of a batch of 0" in str(e.value)
    assert len(empty.select([])) == 0
    empty.free()


# ================================================================ refusals that read the batch
def test_refusals_that_need_a_batch(sassy, searchers):
    L = sassy.lib()
    good = sassy.DeviceReads.from_sequences([b"ACGTACGTAA"])
    long_ = sassy.DeviceReads.from_sequences([b"A" * 513])
    with_n = sassy.DeviceReads.from_sequences([b"ACGTNCGTAA"])
    ptrs = (C.c_char_p * 1)(b"ACGT")
    bounds = (C.c_uint64 * 3)()
    out = C.c_void_p(7)

    def call(s, reads, bounds=bounds, out=C.byref(out)):
        rc = L.sassy_hip_demux_reads(s._h, reads._h, ptrs, 4, 1, 0, 1, 1, 0, None, None, bounds, out)
        return rc, L.sassy_hip_last_error().decode()
    rc, msg = call(searchers["dna"], long_)
    assert rc == -1 and "demux_reads takes reads of at most 512 bytes (SASSY_HIP_OVERLAP_MAX_LEN; the longest has 513)" in msg and out.value is None
    rc, msg = call(searchers["dna"], good, bounds=None)
    assert rc == -1 and "must not be null (out_bounds, out_sorted)" in msg
    rc, msg = call(searchers["dna"], good, out=None)
    assert rc == -1 and "must not be null (out_bounds, out_sorted)" in msg
    out = C.c_void_p(7)
    rc, msg = call(searchers["dna"], with_n, out=C.byref(out))
    assert rc == -1 and "use an iupac searcher" in msg and out.value is None
    with pytest.raises(sassy.SassyHipError) as e:
        good.demux(searchers["dna"], [b"ACGN"])
    assert "barcode 0 holds other bytes than A, C, G, T" in str(e.value)
    with pytest.raises(sassy.SassyHipError) as e:
        good.demux(searchers["dna"], [b"ACGT", b"ACG"])
    assert "one length" in str(e.value)
    d = good.demux(searchers["iupac"], [b"ACGN"], k=0, with_records=True)
    assert d.bounds.tolist() == [0, 1, 1] and d.records[0]["cost"] == 0 and d.reads.download(0) == b"ACGTAA"
    d.free()
    for h in (good, long_, with_n):
        h.free()


# ================================================================ downstream: a mate batch in the order, a search on a sample
def test_the_mate_batch_selected_by_the_order(sassy, searchers):
    rng = np.random.default_rng(31)
    reads = dref.mixed_batch(500, 6, MIXED_BARCODES)
    mates = with_quals(rng, [random_seq(rng, int(rng.integers(0, 160))) for _ in reads])
    h1 = sassy.DeviceReads.from_sequences([s for s, _ in reads], [q for _, q in reads])
    h2 = sassy.DeviceReads.from_sequences([s for s, _ in mates], [q for _, q in mates])
    want = dref.expected_demux("dna", reads, MIXED_BARCODES, k=1)
    d = h1.demux(searchers["dna"], MIXED_BARCODES, k=1)
    assert np.array_equal(d.order, want[1])
    sorted_mates = h2.select(d.order)
    exp = dref.expected_select(mates, want[1].tolist())
    compare_handle(sorted_mates, [s for s, _ in exp], [q for _, q in exp], "mates in the order")
    for s in (0, 3, -1):   # a sample of both, record for record the same pairs
        a, b = d.span(s)
        m = sorted_mates.select(np.arange(a, b, dtype=np.uint64))
        compare_handle(m, [x for x, _ in exp[a:b]], [q for _, q in exp[a:b]], ("mates of sample", s))
        m.free()
    for x in (sorted_mates, d, h1, h2):
        x.free()


def test_hamming_best_pattern_on_a_sample(sassy, searchers):
    rng = np.random.default_rng(41)
    reads = dref.mixed_batch(400, 7, MIXED_BARCODES)
    want = dref.expected_demux("dna", reads, MIXED_BARCODES, k=1)
    d = sassy.demux_reads(searchers["dna"], reads, MIXED_BARCODES, k=1)
    pats = [b"ACGTAC", b"TTGACA", b"GGGTTT"]
    total = 0
    for s in (0, 2, 3, -1):
        a, b = d.span(s)
        host = want[3][a:b]
        sample = d.sample(s)
        compare_handle(sample, host, want[4][a:b], ("sample", s))
        got = searchers["dna"].hamming_best_pattern(pats, sample, 2)
        exp = searchers["dna"].hamming_best_pattern(pats, host, 2)
        assert len(got) == len(exp) and all(np.array_equal(x, y) for x, y in zip(got, exp)), ("best pattern on sample", s)
        total += len(host)
        sample.free()
    assert total > 200
    d.free()
    with pytest.raises(sassy.SassyHipError):
        d2 = sassy.demux_reads(searchers["dna"], reads[:5], MIXED_BARCODES)
        try:
            d2.span(5)
        finally:
            d2.free()
