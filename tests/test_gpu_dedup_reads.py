"""UMI grouping and deduplication of a resident read batch on the device (sassy_amd/csrc/dedup_reads.hip) against its definition
(tests/helpers/dedup_reads_ref.py), against `Searcher.umi_groups` on the host list of windows mapped back, and against
`reads.select(kept)`: every comparison is exact equality -- the columns array to array, the kept reads, the starts and lengths,
the text and quality buffers byte for byte, pads and the 64 spare bytes included, the block table, the longest read, the layout's
size, the stats.  No tolerance anywhere.

Geometry the shapes aim at: the flag, encode, scatter, keep and compaction kernels are a lane per read in workgroups of 256; the
score kernel gives a read eight lanes (32 reads a workgroup); a window is up to 128 bytes at any alignment, fetched as one block
of five 16-byte pieces for m <= 64 and two for m <= 128; the planes are stored at 1, 2 or 4 words each (m <= 32, 64, 128); the
scans run in blocks of 1 024 items; the write kernel is a lane per 64-byte block of the output.  The shapes are the smallest at
which these can go wrong, not a workload."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, ROOT)

import dedup_reads_ref as ddref  # noqa: E402
import demux_reads_ref as dref  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 5  # tests/test_dedup_reads_cpu.py checks that this batch is non-trivial
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


@pytest.fixture(scope="module")
def searchers(sassy):
    return {("dna", False): sassy.Searcher("dna", rc=False), ("iupac", False): sassy.Searcher("iupac", rc=False),
            ("dna", True): sassy.Searcher("dna", rc=True), ("iupac", True): sassy.Searcher("iupac", rc=True)}


def make(sassy, reads):
    paired = bool(reads) and isinstance(reads[0], tuple)
    return sassy.DeviceReads.from_sequences([x[0] for x in reads], [x[1] for x in reads]) if paired else sassy.DeviceReads.from_sequences(reads)


def same_handle(a, b, ctx):
    """two handles hold the same: the tables, both buffers with their pads, rem, longest, text_bytes"""
    assert len(a) == len(b) and a.longest == b.longest and a.text_bytes == b.text_bytes and bool(a.qual_ptr) == bool(b.qual_ptr), (ctx, len(a), len(b))
    for name in ("seq_starts", "seq_lens", "qual_starts", "qual_lens", "id_starts", "id_lens"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (ctx, name)
    assert a.download_text() == b.download_text(), (ctx, "text")
    if a.qual_ptr:
        assert a.download_quality_text() == b.download_quality_text(), (ctx, "quality")
    assert np.array_equal(a.download_rem(), b.download_rem()), (ctx, "rem")


def own_launches(profile, dedup):
    """this unit's kernels: flag, the scan's three, encode, scatter; the dedup call also score, keep, the scan's three, the
    compaction, the layout scan's three, write; in front of them the Dna look"""
    return (16 if dedup else 6) + (profile == "dna")


def check(sassy, searchers, profile, reads, m, ctx, rc=False, helper=True, batch=None, **kw):
    """both calls over a list of (sequence, quality) or of sequences -- or over `batch`, a DeviceReads that holds them -- against
    the helper, against Searcher.umi_groups on the host list of windows, against select(kept); returns the dedup's kept reads"""
    s = searchers[(profile, rc)]
    seqs, quals = ddref.split(reads)
    n = len(seqs)
    have, wins = ddref.windows(seqs, m, kw.get("at", 0), kw.get("end3", False))
    k, method = kw.get("k", 1), kw.get("method", "directional")
    b = batch if batch is not None else make(sassy, reads)
    d = sel = None
    try:
        # ---- the host route's columns, mapped back (and the stats its walk leaves) ----
        label, rep = np.full(n, NONE, dtype=np.uint32), np.full(n, NONE, dtype=np.uint32)
        size, count = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        host_stats = None
        if have:
            l, z, r, c = s.umi_groups(wins, k, method)
            host_stats = s.stats()
            back = np.array(have, dtype=np.uint32)
            label[back], size[back], rep[back], count[back] = back[l], z, back[r], c
        n_unique, n_groups = int((rep == np.arange(n)).sum()), int((label == np.arange(n)).sum())
        kept = ddref.kept_of(label, ddref.scores(reads))
        if helper:  # the definition, where the brute force behind it is affordable
            want = ddref.expected_dedup(profile, reads, m, rc=rc, **kw)
            for name, x, y in zip(("label", "size", "rep", "count"), want[:4], (label, size, rep, count)):
                assert np.array_equal(x, y), (ctx, "helper against the host route", name)
            assert want[4:6] == (n_unique, n_groups) and np.array_equal(want[6], kept), (ctx, want[4:6], n_unique, n_groups)

        # ---- the groups call ----
        g = b.umi_groups(s, m, **kw)
        st = s.stats()
        for name, x, y in zip(("label", "size", "rep", "count"), g[:4], (label, size, rep, count)):
            bad = np.flatnonzero(x != y)
            assert x.dtype == np.uint32 and len(x) == n and not bad.size, (ctx, "umi_groups", name, bad[:3], x[bad[:3]], y[bad[:3]])
        assert g[4:] == (n_unique, n_groups), (ctx, g[4:], n_unique, n_groups)
        if have:
            assert st["scan_launches"] == own_launches(profile, False) + host_stats["scan_launches"], (ctx, st, host_stats)
            for key in ("filtered", "candidates", "hit_blocks", "chunks", "grid"):  # (blocks, the relaxation's launches, is the schedule's)
                assert st[key] == host_stats[key], (ctx, key, st[key], host_stats[key])
            assert (st["blocks"] > 0) == (host_stats["blocks"] > 0), (ctx, st["blocks"], host_stats["blocks"])
            assert st["filtered"] == 12 and st["hit_blocks"] == n_unique and st["text_bytes"] == len(have) * m, (ctx, st)
        else:
            assert st["scan_launches"] == 0 and st["candidates"] == 0, (ctx, st)

        # ---- the dedup call ----
        d = b.dedup(s, m, with_columns=True, **kw)
        st = s.stats()
        for name, x, y in zip(("label", "size", "rep", "count"), (d.label, d.size, d.rep, d.count), (label, size, rep, count)):
            assert np.array_equal(x, y), (ctx, "dedup", name)
        assert (d.n_unique, d.n_groups) == (n_unique, n_groups) and d.kept.dtype == np.uint64 and np.array_equal(d.kept, kept), (ctx, d.kept[:8], kept[:8])
        if have:
            assert st["scan_launches"] == own_launches(profile, True) + host_stats["scan_launches"], (ctx, st, host_stats)
            assert st["filtered"] == 12 and st["hit_blocks"] == n_unique and st["candidates"] == host_stats["candidates"], (ctx, st)
        else:
            assert st["scan_launches"] == 0 and d.reads.text_bytes == 64 and len(d.reads) == 0, (ctx, st)
        sel = b.select(kept)
        same_handle(d.reads, sel, ctx)
        out = dref.expected_select(reads, kept.astype(np.int64).tolist())
        text, qual, starts, rem, longest = dref.layout([x[0] for x in out], [x[1] for x in out] if b.qual_ptr else None)
        assert d.reads.download_text() == text and d.reads.longest == longest and np.array_equal(d.reads.seq_starts, starts), (ctx, "layout")
        assert bool(d.reads.qual_ptr) == bool(b.qual_ptr) and (not b.qual_ptr or d.reads.download_quality_text() == qual), (ctx, "quality")
        assert np.array_equal(d.reads.download_rem(), rem) and not d.reads.id_lens.any(), (ctx, "rem")
        # without columns: the same kept reads
        d2 = b.dedup(s, m, **kw)
        try:
            assert d2.label is None and np.array_equal(d2.kept, kept) and (d2.n_unique, d2.n_groups) == (n_unique, n_groups), ctx
        finally:
            d2.free()
        return kept
    finally:
        for x in (d, sel, None if batch is not None else b):
            if x is not None:
                x.free()


# ================================================================ the definition's own case
def test_the_case_written_out_by_hand(sassy, searchers):
    reads = ddref.hand_batch()
    for profile in ("dna", "iupac"):
        kept = check(sassy, searchers, profile, reads, 4, "hand")
        assert kept.tolist() == ddref.HAND_KEPT["directional"]
        g = make(sassy, reads)
        try:
            label = g.umi_groups(searchers[(profile, False)], 4)[0]
            assert [r for r in range(len(reads)) if label[r] == NONE] == list(ddref.HAND_NO_WINDOW)
        finally:
            g.free()


# ================================================================ read counts: workgroup, score-group and scan-block borders
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025, 4001])
def test_read_counts(sassy, searchers, n):
    check(sassy, searchers, "dna", ddref.seeded_batch(n, SEED), 12, ("n", n))


# ================================================================ key lengths: 1, 2 and 4 words per plane, one and two blocks
@pytest.mark.parametrize("m", [1, 12, 32, 33, 64, 65, 128])
def test_key_lengths_at_both_ends_and_across_block_borders(sassy, searchers, m):
    for at, end3, profile in ((0, False, "dna"), (5, True, "iupac"), (60, False, "iupac"), (122, True, "dna"), (384 - m // 2, False, "dna")):
        letters = b"ACGT" if profile == "dna" else b"ACGTNRYacgtnU"
        reads = ddref.seeded_batch(130, SEED + m, m=m, at=at, end3=end3, letters=letters, n_umis=9)
        # one long read whose window lies deep inside it, and the reads padded so that the window crosses 64-byte borders
        reads = [(s, q) if r % 7 else (s + s[:1] * (300 - min(300, len(s))), q + q[:1] * (300 - min(300, len(s)))) for r, (s, q) in enumerate(reads)]
        reads = [(s[:512], q[:512]) for s, q in reads]
        check(sassy, searchers, profile, reads, m, ("m", m, at, end3, profile), at=at, end3=end3, k=1 if m < 64 else 2)


def test_the_last_window_ends_at_the_handles_last_byte(sassy, searchers):
    """the last read fills its blocks, and its key is its last bytes: the fetch runs up to the 64 spare bytes and no further"""
    rng = np.random.default_rng(3)
    pick = lambda k: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), k).astype(np.uint8))
    for la, m in ((64, 12), (128, 64), (128, 128), (512, 100), (192, 65)):
        key = pick(m)
        reads = [pick(40) + key, pick(7), pick(la - m) + key[:-1] + (b"A" if key[-1:] != b"A" else b"C"), pick(la - m) + key]
        assert len(reads[-1]) == la
        check(sassy, searchers, "dna", reads, m, ("last byte", la, m), end3=True)
        check(sassy, searchers, "dna", with_constant_quality(reads), m, ("last byte, qualities", la, m), end3=True)


def with_constant_quality(seqs):
    return [(s, b"5" * len(s)) for s in seqs]


# ================================================================ degenerate batches
def test_all_identical_all_distinct_and_none_with_a_window(sassy, searchers):
    same = [b"ACGTACGTACGT" + b"T" * (r % 5) for r in range(300)]
    kept = check(sassy, searchers, "dna", same, 12, "identical")
    assert kept.tolist() == [4]                                   # the longest, the first of them
    kept = check(sassy, searchers, "dna", with_constant_quality(same), 12, "identical, qualities")
    assert kept.tolist() == [4]
    # all distinct and pairwise further apart than k: the key spells the read's index in base 4, every digit twice
    distinct = [bytes(b"ACGT"[(r >> (2 * (i // 2))) & 3] for i in range(12)) + b"GG" for r in range(300)]
    kept = check(sassy, searchers, "dna", distinct, 12, "distinct", k=1)
    assert kept.tolist() == list(range(300))
    for method in ddref.uref.METHODS:
        short = [b"ACGT" * (r % 3) for r in range(70)]              # none reaches 12 bytes
        kept = check(sassy, searchers, "iupac", short, 12, ("no window", method), method=method)
        assert kept.size == 0
    assert check(sassy, searchers, "dna", [b"", b""], 1, "empty reads").size == 0


# ================================================================ methods, alphabets, strands, qualities
@pytest.mark.parametrize("method", ["unique", "cluster", "directional"])
def test_the_three_methods(sassy, searchers, method):
    for k in (0, 1, 2, 200):
        check(sassy, searchers, "dna", ddref.seeded_batch(700, SEED, n_umis=40), 12, (method, k), method=method, k=k)


def test_iupac_with_n(sassy, searchers):
    reads = ddref.seeded_batch(600, SEED + 1, m=10, letters=b"ACGTNNacgtnRYU", n_umis=30)
    assert sum(b"N" in s[:10] for s, _ in reads) > 50
    for end3 in (False, True):
        check(sassy, searchers, "iupac", ddref.seeded_batch(600, SEED + 1, m=10, letters=b"ACGTNNacgtnRYU", n_umis=30, end3=end3), 10, ("iupac", end3), end3=end3)


def test_dna_searcher_refuses_other_bytes(sassy, searchers):
    b = make(sassy, [b"ACGTACGTAC", b"ACGNACGTAC"])
    try:
        for call in (lambda: b.umi_groups(searchers[("dna", False)], 4), lambda: b.dedup(searchers[("dna", False)], 4)):
            with pytest.raises(sassy.SassyHipError, match="use an iupac searcher"):
                call()
    finally:
        b.free()


def test_rc_searcher_groups_across_strands(sassy, searchers):
    for profile, m in (("dna", 12), ("iupac", 12), ("dna", 33), ("dna", 70), ("iupac", 128)):
        reads = ddref.seeded_batch(500, SEED + 2, m=m, rc_mix=True, n_umis=25)
        check(sassy, searchers, profile, reads, m, ("rc", profile, m), rc=True)
        check(sassy, searchers, profile, reads, m, ("rc, cluster", profile, m), rc=True, method="cluster", end3=False, at=0)
    # palindromes: their reverse complement is themselves
    pal = [b"ACGT", b"AATT", b"ACGT", b"TTAA", b"AAAA", b"TTTT", b"GATC", b"GTAC", b"AATT", b"TTTT", b"TTTA", b"TAAA"]
    for method in ("cluster", "directional"):
        check(sassy, searchers, "dna", [p + b"CC" * (i % 3) for i, p in enumerate(pal)], 4, ("palindromes", method), rc=True, method=method)
    # the strands differ: without rc, AAAA and TTTT are four apart
    a = check(sassy, searchers, "dna", [b"AAAAC", b"TTTTCC"], 4, "rc on", rc=True, k=0, method="cluster")
    b = check(sassy, searchers, "dna", [b"AAAAC", b"TTTTCC"], 4, "rc off", rc=False, k=0, method="cluster")
    assert a.tolist() == [1] and b.tolist() == [0, 1]


def test_with_and_without_qualities(sassy, searchers):
    with_q = ddref.seeded_batch(900, SEED, n_umis=50)
    without = [s for s, _ in with_q]
    a = check(sassy, searchers, "dna", with_q, 12, "qualities")
    b = check(sassy, searchers, "dna", without, 12, "no qualities")
    assert len(a) == len(b) and not np.array_equal(a, b)        # the same groups, other reads kept: the score differs
    # a long read of low qualities against a short one of high ones: the sum decides, not the length
    reads = [(b"ACGTACGTAAAAAAAA", b"!" * 16), (b"ACGTACGTCC", b"~" * 10)]
    assert check(sassy, searchers, "dna", reads, 8, "sum").tolist() == [1]
    assert check(sassy, searchers, "dna", [s for s, _ in reads], 8, "length").tolist() == [0]
    # 512 bytes of the highest byte: the largest score there is
    reads = [(b"ACGT" * 128, b"\x7e" * 512), (b"ACGT" * 128, b"\x7e" * 511 + b"\x7d"), (b"ACGT" * 100, b"\x7e" * 400)]
    assert check(sassy, searchers, "dna", reads, 128, "largest score", at=100).tolist() == [0]


# ================================================================ handles that other calls made
def test_handles_made_by_trim_and_by_demux(sassy, searchers):
    s = searchers[("dna", False)]
    adapter = b"AGATCGGAAGAGC"
    base = ddref.seeded_batch(400, SEED + 3, n_umis=20)
    reads = [(q_s + (adapter if r % 3 == 0 else b""), q_q + (b"I" * len(adapter) if r % 3 == 0 else b"")) for r, (q_s, q_q) in enumerate(base)]
    src = make(sassy, reads)
    trimmed = d = sample = None
    try:
        trimmed = s.trim_reads(src, [adapter], min_overlap=5, k=0)
        got = [(trimmed.download(i), trimmed.quality(i)) for i in range(len(trimmed))]
        assert sum(len(a[0]) != len(b[0]) for a, b in zip(got, reads)) > 100
        check(sassy, searchers, "dna", got, 12, "trimmed", batch=trimmed)
        barcodes = [b"ACGTAC", b"TTGGCC"]
        tagged = [(barcodes[r % 2] + x, b"F" * 6 + y) for r, (x, y) in enumerate(base)]
        tagged_reads = make(sassy, tagged)
        try:
            d = tagged_reads.demux(s, barcodes, k=0)
        finally:
            tagged_reads.free()
        for which in (0, 1):
            sample = d.sample(which)
            got = [(sample.download(i), sample.quality(i)) for i in range(len(sample))]
            assert got == [(x, y) for r, (x, y) in enumerate(base) if r % 2 == which]
            check(sassy, searchers, "dna", got, 12, ("sample", which), batch=sample)
            sample.free()
            sample = None
    finally:
        for x in (src, trimmed, d, sample):
            if x is not None:
                x.free()


def test_module_level_call_and_refusals_that_read_the_batch(sassy, searchers):
    s = searchers[("dna", False)]
    reads = ddref.seeded_batch(100, SEED)
    d = sassy.dedup_reads(s, reads, 12, with_columns=True)
    try:
        want = ddref.expected_dedup("dna", reads, 12)
        assert np.array_equal(d.kept, want[6]) and np.array_equal(d.label, want[0]) and d.n_groups == want[5]
    finally:
        d.free()
    long_reads = make(sassy, [b"A" * 513])
    try:
        with pytest.raises(sassy.SassyHipError, match="at most 512 bytes"):
            long_reads.dedup(s, 12)
        with pytest.raises(sassy.SassyHipError, match="at most 512 bytes"):
            long_reads.umi_groups(s, 12)
    finally:
        long_reads.free()


# ================================================================ the command
def test_dedup_command_files_with_a_mate(sassy, tmp_path):
    reads = ddref.seeded_batch(300, SEED, n_umis=15)
    reads = [(s, q) if s else (b"A", b"I") for s, q in reads]      # (FASTQ on disk holds no empty record here)
    fq = lambda rs, tag: b"".join(b"@%s%d x\n%s\n+\n%s\n" % (tag, i, s, q) for i, (s, q) in enumerate(rs))
    mates = [(bytes(b"ACGT"[(i + j) % 4] for j in range(20 + i % 9)), b"H" * (20 + i % 9)) for i in range(len(reads))]
    (tmp_path / "r1.fq").write_bytes(fq(reads, b"r"))
    (tmp_path / "r2.fq").write_bytes(fq(mates, b"m"))
    p = subprocess.run([sys.executable, "-m", "sassy_amd", "dedup", str(tmp_path / "r1.fq"), "--umi-len", "12", "-o", str(tmp_path / "o1.fq"),
                        "--mate", str(tmp_path / "r2.fq"), "--mate-out", str(tmp_path / "o2.fq"), "--tsv", str(tmp_path / "o.tsv")],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    label, size, rep, count, n_unique, n_groups, kept, out = ddref.expected_dedup("dna", reads, 12)
    kept = kept.astype(np.int64).tolist()
    assert (tmp_path / "o1.fq").read_bytes() == b"".join(b"@r%d x\n%s\n+\n%s\n" % (r, *reads[r]) for r in kept)
    assert (tmp_path / "o2.fq").read_bytes() == b"".join(b"@m%d x\n%s\n+\n%s\n" % (r, *mates[r]) for r in kept)
    rows = (tmp_path / "o.tsv").read_text().splitlines()
    assert rows[0] == "read_id\tlabel_id\tsize\tcount\tkept" and len(rows) == 1 + len(reads)
    for r, row in enumerate(rows[1:]):
        lab = "-" if label[r] == NONE else f"r{label[r]} x"
        assert row == f"r{r} x\t{lab}\t{size[r]}\t{count[r]}\t{int(r in kept)}", (r, row)
