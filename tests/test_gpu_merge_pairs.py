"""The paired-end merge on the device (sassy_amd/csrc/merge_pairs.hip) and the kept qualities of a read batch
(SASSY_HIP_KEEP_QUALITY, sassy_amd/csrc/fastq_reads.hip) against their definitions (tests/helpers/merge_pairs_ref.py,
fastq_ref.py): every comparison is exact equality -- the merged text and quality buffers byte for byte, pads and the 64 spare
bytes included, the block table, the starts and lengths, the record table and the overlap records.  No tolerance anywhere.

Geometry the shapes aim at: the write kernel is a lane per 64-byte block of the OUTPUT; a's bytes are aligned 16-byte loads,
R2's come from an address of any alignment mod 16 (and in front of the buffer for a first read) through a shift and a word
reversal; the layout scan is the parse's, in blocks of 1 024 records.  The shapes are the smallest at which these can go
wrong, not a workload."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import fastq_ref  # noqa: E402
import merge_pairs_ref as mref  # noqa: E402
import read_overlaps_ref as oref  # noqa: E402

pytestmark = pytest.mark.gpu


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


def random_qual(rng, n):
    return bytes(rng.integers(33, 75, n).astype(np.uint8))


def with_quals(rng, seqs):
    return [(s, random_qual(rng, len(s))) for s in seqs]


def compare(merged, records, want, ctx):
    """a merged handle and the call's records against (records, sequences, qualities) of the helper: everything the handle holds"""
    want_records, seqs, quals = want
    starts, lens, text = mref.layout_of(seqs)
    qual = mref.layout_of(quals)[2]
    assert len(merged) == len(seqs), (ctx, len(merged), len(seqs))
    if records is not None:
        bad = np.flatnonzero(records != want_records)
        assert records.dtype == want_records.dtype and not bad.size, (ctx, "record", bad[:1], records[bad[:1]], want_records[bad[:1]])
    for name, got, exp in (("seq_start", merged.seq_starts, starts), ("seq_len", merged.seq_lens, lens), ("qual_start", merged.qual_starts, starts),
                           ("qual_len", merged.qual_lens, lens), ("id_start", merged.id_starts, 0 * lens), ("id_len", merged.id_lens, 0 * lens)):
        bad = np.flatnonzero(got != exp)
        assert not bad.size, (ctx, name, "pair", int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
    assert merged.longest == (int(lens.max()) if len(lens) else 0) and merged.text_bytes == text.size and merged.ptr and merged.qual_ptr, ctx
    for what, got, exp in (("text", merged.download_text(), text), ("quality", merged.download_quality_text(), qual)):
        got = np.frombuffer(got, dtype=np.uint8)
        diff = np.flatnonzero(got != exp)
        if diff.size:
            at = int(diff[0])
            pair = int(np.searchsorted(starts, at, side="right")) - 1
            pytest.fail(f"{ctx}: {what}: first differing byte {at} of {exp.size} (block {at // 64}), pair {pair}, column {at - int(starts[pair])} of "
                        f"{int(lens[pair])}, record {want_records[pair].tolist()}: got {int(got[at])}, want {int(exp[at])}")
    assert np.array_equal(merged.download_rem(), mref.rem_of(starts, lens)), (ctx, "rem")


def check(searchers, profile, pairs1, pairs2, ctx, **kw):
    """the call over lists of (sequence, quality) against the helper"""
    merged, records = searchers[profile].merge_pairs(pairs1, pairs2, with_overlaps=True, **kw)
    want = mref.expected_merge(profile, pairs1, pairs2, **kw)
    try:
        compare(merged, records, want, (ctx, profile, kw))
    finally:
        merged.free()
    return want


# ================================================================ kept qualities
def fastq_of(seqs, quals, eol=b"\n", final=True, tag=b"r"):
    raw = b"".join(b"@%s%d" % (tag, i) + eol + s + eol + b"+" + eol + q + eol for i, (s, q) in enumerate(zip(seqs, quals)))
    return raw if final or not raw else raw[:-len(eol)]


def test_kept_qualities_lie_in_the_layout_of_the_text(sassy):
    rng = np.random.default_rng(1)
    lengths = [0, 1, 63, 64, 65, 128, 129]
    seqs = [random_seq(rng, n, b"ACGTN") for n in lengths]
    quals = [bytes(rng.integers(33, 127, n).astype(np.uint8)) for n in lengths]
    L = sassy.lib()
    for eol in (b"\n", b"\r\n"):
        for order in (list(range(7)), list(range(7))[::-1], [3, 0, 0, 6, 0]):
            for final in (True, False):
                if not final and not lengths[order[-1]]:
                    continue  # (an empty last quality line exists only with its line end)
                raw = fastq_of([seqs[i] for i in order], [quals[i] for i in order], eol, final)
                ctx = (eol, order, final)
                plain, kept = sassy.DeviceReads(raw), sassy.DeviceReads(raw, keep_quality=True)
                buf = sassy.DeviceBuffer((len(raw) + 63) // 64 * 64)
                buf.upload(raw)
                dev = sassy.DeviceReads(sassy.DeviceText(buf.ptr, len(raw), owner=buf), keep_quality=True)
                want = mref.quality_layout(raw)
                for h in (kept, dev):
                    assert h.qual_ptr and h.qual_ptr % 64 == 0 and L.sassy_hip_reads_quality(h._handle()) == h.qual_ptr, ctx
                    got = np.frombuffer(h.download_quality_text(), dtype=np.uint8)
                    assert got.size == want.size == h.text_bytes and np.array_equal(got, want), (ctx, np.flatnonzero(got != want)[:3])
                    assert [h.quality(i) for i in range(len(h))] == [quals[i] for i in order], ctx
                # without the flag: no buffer, and everything else as under it
                assert plain.qual_ptr == 0 and L.sassy_hip_reads_quality(plain._handle()) is None, ctx
                with pytest.raises(sassy.SassyHipError, match="were not kept"):
                    plain.download_quality_text()
                for h in (kept, dev):
                    assert h.download_text() == plain.download_text() and np.array_equal(h.download_rem(), plain.download_rem()), ctx
                    for col in ("id_starts", "id_lens", "seq_starts", "seq_lens", "qual_starts", "qual_lens"):
                        assert np.array_equal(getattr(h, col), getattr(plain, col)), (ctx, col)
                    assert h.longest == plain.longest and h.text_bytes == plain.text_bytes
                assert [plain.quality(i) for i in range(len(plain))] == [quals[i] for i in order], ctx  # (out of the raw bytes)
                for h in (plain, kept, dev, buf):
                    h.free()
    # no record at all: the 64 spare bytes, in both buffers
    empty = sassy.DeviceReads(b"", keep_quality=True)
    assert empty.text_bytes == 64 and empty.download_quality_text() == bytes(64) and len(empty) == 0
    empty.free()
    # from_sequences keeps the qualities it is given, and none otherwise
    a, b = sassy.DeviceReads.from_sequences([b"ACGT", b""], [b"IJKL", b""]), sassy.DeviceReads.from_sequences([b"ACGT", b""])
    assert a.qual_ptr and not b.qual_ptr and a.quality(0) == b"IJKL" and a.quality(1) == b"" and b.quality(0) == b""
    a.free(), b.free()


def test_a_quality_of_another_length_is_refused_under_the_flag_only_and_behind_the_older_verdicts(sassy):
    good = [b"@g%d\n%s\n+\n%s\n" % (i, b"ACGT" * 25, b"I" * 100) for i in range(2100)]  # (three blocks of the record scan)
    for bad in ([1500], [2099, 1030, 1029], [0, 5]):
        recs = list(good)
        for i in bad:
            recs[i] = b"@g%d\n%s\n+\n%s\n" % (i, b"ACGT" * 25, b"I" * (99 + 2 * (i % 2)))
        raw = b"".join(recs)
        with pytest.raises(sassy.SassyHipError, match=r"record %d: its quality is not as long as its sequence \(SASSY_HIP_KEEP_QUALITY" % min(bad)):
            sassy.DeviceReads(raw, keep_quality=True)
        plain = sassy.DeviceReads(raw)  # the length is reported and not compared
        assert int(plain.qual_lens[min(bad)]) in (99, 101) and len(plain) == 2100
        plain.free()
        # a malformed file keeps its old message, wherever the bad quality lies
        for cut, word in ((raw + b"@cut\nAC\n", "record 2100: it has 2 of its four lines"), (raw.replace(b"\n+\n", b"\n-\n", 1), "record 0: its third line"),
                          (b"".join(recs[:2050]) + b"g" + b"".join(recs[2050:])[1:], "record 2050: its first line")):
            for keep in (False, True):
                with pytest.raises(sassy.SassyHipError, match=word):
                    sassy.DeviceReads(cut, keep_quality=keep)
    ok = sassy.DeviceReads(b"".join(good), keep_quality=True)  # (and the device is fine afterwards)
    assert len(ok) == 2100 and ok.quality(2099) == b"I" * 100
    ok.free()


# ================================================================ the merge
def test_the_three_hand_cases(sassy, searchers):
    for profile in ("dna", "iupac"):
        for case in mref.HAND:
            records, seqs, quals = check(searchers, profile, [(case["r1"], case["q1"])], [(case["r2"], case["q2"])], "hand", **mref.HAND_CALL)
            assert (tuple(records[0].tolist()), seqs[0], quals[0]) == (case["record"], case["merged"], case["quality"])
    merged = searchers["dna"].merge_pairs([(c["r1"], c["q1"]) for c in mref.HAND], [(c["r2"], c["q2"]) for c in mref.HAND], **mref.HAND_CALL)
    assert [merged.download(i) for i in range(3)] == [c["merged"] for c in mref.HAND]
    assert [merged.quality(i) for i in range(3)] == [c["quality"] for c in mref.HAND]
    with pytest.raises(sassy.SassyHipError, match="the ids are R1's"):
        merged.id(0)
    assert searchers["dna"].stats()["candidates"] == 3 and searchers["dna"].stats()["scan_launches"] == 5
    merged.free()


@pytest.mark.parametrize("profile", ["dna", "iupac"])
def test_every_pair_of_lengths_up_to_70_with_a_planted_overlap(searchers, profile):
    rng = np.random.default_rng(21)
    r1s, r2s = [], []
    for la in range(1, 71):
        for lb in range(1, 71):
            d = int(rng.integers(-(lb - 1), la))  # any offset that has an overlap
            ov = min(la, d + lb) - max(0, d)
            a, r2 = oref.planted_pair(rng, profile, la, lb, d, subs=int(rng.integers(0, 3)) if ov >= 10 else 0)
            r1s.append(a)
            r2s.append(r2)
    records, seqs, _ = check(searchers, profile, with_quals(rng, r1s), with_quals(rng, r2s), "70 x 70", min_overlap=3, k=2, max_permille=250)
    assert sum(1 for s in seqs if s) > 3500 and (records["offset"] < 0).sum() > 500 and (records["mismatches"] > 0).sum() > 300


def test_merged_lengths_around_the_blocks_offsets_at_the_extremes_and_contained_reads(searchers):
    rng = np.random.default_rng(22)
    mo = 10
    shapes = []
    for L in (63, 64, 65, 127, 128, 129):          # merged length L out of two reads that overlap in 20 rows
        la = L // 2 + 10
        shapes.append((la, L - la + 20, la - 20))
        shapes.append((L, L + 7, -7))               # ... and as a read-through: L = ov = la
    shapes.append((512, 512, 502))                  # 1 014 = 512 + 512 - 10, an overlap of min_overlap rows: sixteen blocks, the last of 54 bytes
    la, lb = 150, 130
    shapes += [(la, lb, d) for d in (-(lb - 1) + mo - 1, -1, 0, 1, la - mo)]
    shapes += [(200, 60, 70), (200, 60, 0), (200, 60, 140), (60, 200, -70), (60, 200, -140), (60, 200, 0)]  # b in a, a in b
    r1s, r2s = zip(*(oref.planted_pair(rng, "dna", la, lb, d, subs=(la + lb) % 2) for la, lb, d in shapes))
    for profile in ("dna", "iupac"):
        records, seqs, _ = check(searchers, profile, with_quals(rng, r1s), with_quals(rng, r2s), "shapes", min_overlap=mo, k=3, max_permille=200)
        assert records["offset"].tolist() == [d for _, _, d in shapes] and (records["n_accepted"] > 0).all()
        assert [len(s) for s in seqs[:13]] == [63, 63, 64, 64, 65, 65, 127, 127, 128, 128, 129, 129, 1014]


def test_sources_at_every_alignment_mod_16(searchers):
    """R2's bytes of a block begin at start2 + lb - 64 + d - 64 block: every residue mod 16 through lb + d, and behind reads of
    1 .. 16 bases, which move the pair through the handles (and the first pair reads in front of R2's buffer)."""
    rng = np.random.default_rng(23)
    r1s, r2s = [], []
    for t in range(1, 17):
        la, lb = 90, 70 + t
        a, r2 = oref.planted_pair(rng, "dna", la, lb, 40 + (t * 7) % 16, subs=t % 3)
        r1s += [a, random_seq(rng, t)]
        r2s += [r2, random_seq(rng, 17 - t)]
        a, r2 = oref.planted_pair(rng, "dna", 60 + t, 100, -(t + 3))   # read-through
        r1s.append(a)
        r2s.append(r2)
    for profile in ("dna", "iupac"):
        records, _, _ = check(searchers, profile, with_quals(rng, r1s), with_quals(rng, r2s), "alignments", min_overlap=12, k=2, max_permille=200)
        assert len({(len(r2s[i]) + int(records[i]["offset"])) % 16 for i in range(len(r1s)) if records[i]["n_accepted"]}) == 16


def test_consensus_corners(searchers):
    a = b"ACGTTGCAAGCTCAGGTCAT"  # (no repeat: no other offset comes near the true one)
    r2 = oref.revcomp("dna", a)
    n = len(a)

    def one(profile, r1, q1, r2, q2, **kw):
        kw = dict(dict(min_overlap=10, k=10, max_permille=1000), **kw)
        _, seqs, quals = check(searchers, profile, [(r1, q1)], [(r2, q2)], "corner", **kw)
        return seqs[0], quals[0]

    # equal bytes: the higher quality, whichever read has it
    qa, qb = bytes([40, 50, 60] + [45] * (n - 3)), bytes([45] * (n - 3) + [60, 50, 40])   # (qb is R2's: reversed, b's is 40, 50, 60, 45 ...)
    s, q = one("dna", a, qa, r2, qb)
    assert s == a and q == bytes([40, 50, 60] + [45] * (n - 3))
    qb = bytes([45] * (n - 3) + [50, 50, 50])
    s, q = one("dna", a, qa, r2, qb)
    assert q[:3] == bytes([50, 50, 60])   # qa <, =, > qb
    # unequal bytes, column 0 .. 5: qa <, =, > qb, and differences of 0, 1, 2 and 93
    b = bytearray(a)
    for i in range(6):
        b[i] = b"ACGT"[(b"ACGT".index(a[i]) + 1) % 4]
    r2x = oref.revcomp("dna", bytes(b))
    qa = bytes([40, 40, 41, 42, 126, 33] + [50] * (n - 6))
    qbb = bytes([41, 40, 40, 40, 33, 126] + [50] * (n - 6))   # b's qualities; R2's are these reversed
    s, q = one("dna", a, qa, r2x, qbb[::-1])
    assert s[:6] == bytes([b[0], a[1], a[2], a[3], a[4], b[5]]) and s[6:] == a[6:]
    assert q[:6] == bytes([35, 35, 35, 35, 126, 126]) and q[6:] == bytes([50] * (n - 6))
    # Iupac: N against a base is a match for the overlap and a difference for the consensus; the higher quality decides
    an = a[:4] + b"N" + a[5:]
    s, q = one("iupac", an, bytes([50] * 4 + [60] + [50] * 15), r2, bytes([40] * n), k=0, max_permille=0)
    assert s == an and q[4] == 33 + 20
    s, q = one("iupac", an, bytes([50] * 4 + [35] + [50] * 15), r2, bytes([40] * n), k=0, max_permille=0)
    assert s == a and q[4] == 33 + 5
    # dna: a lower-case letter matches its upper case (one 2-bit code) and differs from it as a byte; R2's lower case is not complemented
    al = a[:4] + a[4:5].lower() + a[5:]
    s, q = one("dna", al, bytes([50] * n), r2, bytes([50] * n), k=0, max_permille=0)
    assert s == al and q[4] == 35
    s, q = one("dna", a, bytes([50] * n), r2[:3] + b"c" + r2[4:], bytes([51] * n), k=20)
    assert s[n - 4] == ord("c") and q[n - 4] == 35


def test_empty_and_unmerged_pairs_at_every_position_of_a_record_block(searchers):
    rng = np.random.default_rng(24)
    n = 1025
    r1s, r2s = [], []
    for i in range(n):
        a, r2 = oref.planted_pair(rng, "dna", 30 + i % 40, 25 + i % 11, 12 + i % 5)
        r1s.append(a)
        r2s.append(r2)
    unmerged = random_seq(rng, 30), oref.revcomp("dna", random_seq(rng, 30))
    for holes in ([0], [n - 1], [1023], [1024], [1023, 1024], [0, 1, 2, 500, 501, 1022, 1023], list(range(1000, 1025)), list(range(0, 1024))):
        x, y = list(r1s), list(r2s)
        for j, i in enumerate(holes):
            x[i], y[i] = (b"", y[i]) if j % 3 == 0 else (x[i], b"") if j % 3 == 1 else unmerged
        _, seqs, _ = check(searchers, "dna", with_quals(rng, x), with_quals(rng, y), ("holes", holes[:3], len(holes)), min_overlap=10, k=0, max_permille=0)
        assert [i for i, s in enumerate(seqs) if not s] == holes
    # no pair merged: the 64 spare bytes alone; and no pair at all
    for pairs in ([unmerged] * 3, [(b"", b"")] * 2, [(b"", b"ACGT"), (b"ACGT", b"")], []):
        p1, p2 = with_quals(rng, [p[0] for p in pairs]), with_quals(rng, [p[1] for p in pairs])
        merged, records = searchers["dna"].merge_pairs(p1, p2, with_overlaps=True)
        assert len(merged) == len(pairs) and merged.text_bytes == 64 and merged.download_text() == bytes(64) == merged.download_quality_text()
        assert merged.longest == 0 and not merged.seq_lens.any() and not records["n_accepted"].any() and searchers["dna"].stats()["candidates"] == 0
        assert searchers["dna"].stats()["scan_launches"] == (5 if pairs else 0)
        compare(merged, records, mref.expected_merge("dna", p1, p2), ("nothing merged", len(pairs)))
        merged.free()


def test_the_layout_scan_is_the_parses_and_its_second_level_is_reached_there():
    """The merged lengths go through fastq_reads.hip's record scan as a second source of lengths: one sum kernel, one top
    kernel and one write kernel, each defined once, and the merge unit has no kernel but its write kernel.  So the top
    kernel's per == 2 path (more than 1 024 blocks of 1 024 records) is the one
    tests/test_gpu_fastq_reads.py::test_the_top_level_of_every_scan reaches with the parse."""
    code = re.sub(r"//.*", "", open(os.path.join(ROOT, "sassy_amd", "csrc", "fastq_reads.hip")).read())
    for kernel in ("fastq_rec_sum_kernel", "fastq_rec_top_kernel", "fastq_rec_write_kernel"):
        assert len(re.findall(r"__global__[^;{]*\b" + kernel + r"\(", code)) == 1, kernel
    assert "struct MergedSource" in code and "int reads_layout_merged(" in code
    merge = re.sub(r"//.*", "", open(os.path.join(ROOT, "sassy_amd", "csrc", "merge_pairs.hip")).read())
    assert merge.count("__global__") == 1 and "merge_write_kernel" in merge and "__shared__" not in merge   # no scan of its own
    import test_gpu_fastq_reads as parse_tests
    assert callable(parse_tests.test_the_top_level_of_every_scan)


# ================================================================ the merged handle in the rest of the project
@pytest.fixture(scope="module")
def batch():
    """70 pairs: ordinary overlaps, read-throughs, empty reads and pairs without an overlap; the helper's result, once."""
    rng = np.random.default_rng(25)
    r1s, r2s = [], []
    for i in range(70):
        la, lb = int(rng.integers(30, 200)), int(rng.integers(30, 200))
        d = int(rng.integers(0, la - 15)) if i % 3 else -int(rng.integers(1, lb - 15))
        a, r2 = oref.planted_pair(rng, "dna", la, lb, d, subs=i % 3)
        if i % 10 == 9:
            a, r2 = (b"", r2) if i % 20 == 9 else (random_seq(rng, la), oref.revcomp("dna", random_seq(rng, lb)))
        r1s.append(a)
        r2s.append(r2)
    p1, p2 = with_quals(rng, r1s), with_quals(rng, r2s)
    return p1, p2, mref.expected_merge("dna", p1, p2, 10, 5, 200)


def test_the_batch_calls_take_the_merged_handle(sassy, searchers, batch):
    p1, p2, (want_records, seqs, quals) = batch
    s = searchers["dna"]
    merged = s.merge_pairs(p1, p2, 10, 5, 200)
    try:
        assert sum(1 for x in seqs if not x) >= 7 and sum(1 for x in seqs if x) >= 55
        pats = [seqs[0][5:17], seqs[3][:12], oref.revcomp("dna", seqs[4][-12:]), b"ACGTACGTACGT"]
        host, dev = sassy.Searcher("dna", rc=True), sassy.Searcher("dna", rc=True)
        key = lambda m: (m.pattern_idx, m.text_idx, m.text_start, m.text_end, m.cost, m.strand, m.cigar)  # noqa: E731
        for call in (lambda x, t: [a.tolist() for a in x.hamming_best_pattern(pats, t, 2)],
                     lambda x, t: [key(m) for m in x.search_hamming_many(pats, t, 2)],
                     lambda x, t: x.hamming_counts_many(pats, t, 2).tolist(),
                     lambda x, t: [key(m) for m in x.search_many(pats, t, 2)],
                     lambda x, t: [a.tolist() for a in x.min_costs(pats, t, 2, strands=True)]):
            a, b = call(host, seqs), call(dev, merged)
            assert a == b and len(a) > 0
        assert min(host.hamming_best_pattern(pats, seqs, 2)[0].tolist()) == 0 and len(host.search_many(pats, seqs, 2)) >= 3
        compare(merged, None, (want_records, seqs, quals), "after the batch calls")  # the handle is only read
    finally:
        merged.free()


def test_overlaps_inputs_lists_and_layouts(sassy, searchers, batch):
    p1, p2, want = batch
    s = searchers["dna"]
    raw1 = fastq_of([x[0] for x in p1], [x[1] for x in p1], b"\r\n", tag=b"pair")
    raw2 = fastq_of([x[0] for x in p2], [x[1] for x in p2], b"\n", final=False, tag=b"a much longer id for the mate ")
    h1, h2 = sassy.DeviceReads(raw1, keep_quality=True), sassy.DeviceReads(raw2, keep_quality=True)
    l1 = sassy.DeviceReads.from_sequences([x[0] for x in p1], [x[1] for x in p1])
    try:
        state = lambda h: (h.download_text(), h.download_quality_text(), h.download_rem().tolist(), h.seq_starts.tolist(), h.seq_lens.tolist())  # noqa: E731
        before = state(h1), state(h2)
        merged, records = s.merge_pairs(h1, h2, 10, 5, 200, with_overlaps=True)
        assert np.array_equal(records, s.read_overlaps(h1, h2, 10, 5, 200)) and (state(h1), state(h2)) == before
        compare(merged, records, want, "resident")
        merged.free()
        for x, y in ((l1, h2), (p1, p2), (h1, p2)):  # lists, handles of either making, mixed: one result
            merged = s.merge_pairs(x, y, 10, 5, 200)
            compare(merged, None, want, "mixed inputs")
            merged.free()
        assert (state(h1), state(h2)) == before
        # another searcher on the same handles
        merged = searchers["iupac"].merge_pairs(h1, h2, 10, 5, 200)
        compare(merged, None, mref.expected_merge("iupac", p1, p2, 10, 5, 200), "iupac on the same handles")
        merged.free()
        # a merged handle as an input of the next merge: it keeps its qualities, and its layout is another one than r2's
        merged = s.merge_pairs(h1, h2, 10, 5, 200)
        tails = [(oref.revcomp("dna", x[-20:]), q[:20]) for x, q in zip(want[1], want[2])]
        again, records = s.merge_pairs(merged, tails, 10, 0, 0, with_overlaps=True)
        compare(again, records, mref.expected_merge("dna", list(zip(want[1], want[2])), tails, 10, 0, 0), "a merged handle as r1")
        again.free(), merged.free()
    finally:
        for h in (h1, h2, l1):
            h.free()


# ================================================================ refusals
def test_refusals_that_read_the_handles(sassy, searchers):
    import ctypes as C
    L = sassy.lib()
    s = searchers["dna"]
    kept = sassy.DeviceReads.from_sequences([b"ACGTACGTACGT"] * 2, [b"IIIIIIIIIIII"] * 2)
    plain = sassy.DeviceReads.from_sequences([b"ACGTACGTACGT"] * 2)
    three = sassy.DeviceReads.from_sequences([b"ACGT"] * 3, [b"IIII"] * 3)
    long_ = sassy.DeviceReads.from_sequences([b"A" * 513, b"ACGT"], [b"I" * 513, b"IIII"])
    other = sassy.DeviceReads.from_sequences([b"ACGTACGTACGN"] * 2, [b"IIIIIIIIIIII"] * 2)

    def refused(searcher, r1, r2, code, word, flags=0, min_overlap=10, null_out=False):
        out = C.c_void_p(7)
        rc = L.sassy_hip_merge_pairs(searcher._h, r1._handle(), r2._handle(), min_overlap, 512, 200, flags, None, None if null_out else C.byref(out))
        msg = L.sassy_hip_last_error().decode()
        assert rc == code and word in msg and (null_out or out.value is None), (rc, msg, word, out.value)

    try:
        refused(s, plain, kept, -1, "r1 was parsed without SASSY_HIP_KEEP_QUALITY")
        refused(s, kept, plain, -1, "r2 was parsed without SASSY_HIP_KEEP_QUALITY")
        refused(s, kept, three, -1, "r1 holds 2 reads, r2 holds 3")
        refused(s, long_, kept, -1, "at most 512 bytes")
        refused(s, kept, long_, -1, "at most 512 bytes")
        refused(sassy.Searcher("ascii", rc=False), kept, kept, -1, "have no complement")
        refused(s, other, kept, -1, "r1 holds other bytes than A, C, G, T")
        refused(s, kept, other, -1, "r2 holds other bytes than A, C, G, T")
        refused(s, kept, kept, -1, "merge_pairs takes no flags", flags=sassy.KEEP_QUALITY)
        refused(s, kept, kept, -1, "min_overlap must be at least 1", min_overlap=0)
        refused(s, kept, kept, -1, "must not be null (out_merged)", null_out=True)
        refused(s, plain, kept, -1, "SASSY_HIP_KEEP_QUALITY", null_out=True)   # the qualities come first
        with pytest.raises(sassy.SassyHipError, match="KEEP_QUALITY"):
            s.merge_pairs(plain, kept)
        with pytest.raises(sassy.SassyHipError, match="r1 holds 2 reads, r2 holds 3"):
            s.merge_pairs(kept, three)
        # and the call still works afterwards, under iupac with the N as well
        merged = searchers["iupac"].merge_pairs(other, kept, 4)
        assert len(merged) == 2
        merged.free()
        merged = s.merge_pairs(kept, kept, 4)
        assert len(merged) == 2
        merged.free()
    finally:
        for h in (kept, plain, three, long_, other):
            h.free()
    with pytest.raises(sassy.SassyHipError, match="freed"):
        s.merge_pairs(kept, kept)


# ================================================================ the CLI
def test_cli_merge_writes_the_helpers_records_and_the_unmerged_pairs(sassy, batch, tmp_path, monkeypatch, capsysbinary):
    from sassy_amd import cli
    p1, p2, (want_records, seqs, quals) = batch
    raw1 = [b"@pair%d x\r\n%s\r\n+pair%d\r\n%s\r\n" % (i, s, i, q) for i, (s, q) in enumerate(p1)]
    raw2 = [b"@mate%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(p2)]
    f1, f2 = tmp_path / "r1.fq", tmp_path / "r2.fq"
    f1.write_bytes(b"".join(raw1))
    f2.write_bytes(b"".join(raw2))
    ids = ["pair%d x" % i for i in range(len(p1))]
    want = b"".join(b"@" + i.encode() + b"\n" + s + b"\n+\n" + q + b"\n" for i, s, q in zip(ids, seqs, quals) if s)
    holes = [i for i, s in enumerate(seqs) if not s]
    out, u1, u2 = tmp_path / "m.fq", tmp_path / "u1.fq", tmp_path / "u2.fq"
    for batch_bytes in (cli.BATCH_BYTES, 3000):  # (the second: many chunks)
        monkeypatch.setattr(cli, "BATCH_BYTES", batch_bytes)
        argv = ["merge", str(f1), str(f2), "--min-overlap", "10", "-k", "5", "--max-permille", "200"]
        assert cli.main(argv + ["-o", str(out), "--unmerged1", str(u1), "--unmerged2", str(u2), "--tsv"]) == 0
        assert out.read_bytes() == want
        assert u1.read_bytes() == b"".join(raw1[i] for i in holes) and u2.read_bytes() == b"".join(raw2[i] for i in holes)
        rows = (tmp_path / "m.fq.tsv").read_text()
        assert rows == cli.OVERLAP_HEADER + "".join(cli.overlap_rows(ids, want_records, [len(x[0]) for x in p1], [len(x[0]) for x in p2]))
        capsysbinary.readouterr()
        assert cli.main(argv) == 0
        assert capsysbinary.readouterr().out == want
    # reads_to_fastq of a merged handle is what the CLI wrote
    merged = sassy.Searcher("dna", rc=False).merge_pairs(p1, p2, 10, 5, 200)
    assert sassy.reads_to_fastq(merged, ids) == want
    merged.free()
    f2.write_bytes(b"".join(raw2[:-1]))
    with pytest.raises(ValueError, match="different record counts"):
        cli.main(["merge", str(f1), str(f2), "-o", str(out)])
