"""FASTQ parse on the device and the Hamming batch calls over its read batch (sassy_amd/csrc/fastq_reads.hip) against the
definition (tests/helpers/fastq_ref.py) and against the host-text siblings.

The parse: every case compares the whole result -- the six columns of the table, the longest read and the device buffer byte
for byte: every read's sequence, the zero pads and the 64 spare bytes.  Geometry the shapes aim at: 64 bytes per lane, 4 KiB
per tile (a wavefront), 64 KiB per super-tile (a workgroup of the count pass), one workgroup of 1 024 threads over the
super-tile counts; the record scan works in blocks of 1 024 records, one workgroup of 1 024 threads above them; the copy is
a lane per 64-byte block of the output.  The batch calls: each must return what its _many sibling returns for the host list
of the same sequences, and a small case is held against tests/helpers/hamming_many_ref.py and hamming_counts_ref.py directly."""
import contextlib
import functools
import gzip
import io
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import fastq_ref  # noqa: E402
import hamming_counts_ref as cref  # noqa: E402
import hamming_many_ref as mref  # noqa: E402

pytestmark = pytest.mark.gpu

COLUMNS = (("id_starts", "id_start"), ("id_lens", "id_len"), ("seq_starts", "seq_start"), ("seq_lens", "seq_len"),
           ("qual_starts", "qual_start"), ("qual_lens", "qual_len"))


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


def fastq_of(seqs, eol=b"\n", final=True):
    raw = b"".join(b"@r%d" % i + eol + s + eol + b"+" + eol + b"I" * len(s) + eol for i, s in enumerate(seqs))
    return raw if final or not raw else raw[:-len(eol)]


def compare(sassy, reads, raw, ctx):
    """the table, column by column, the longest read and the whole device buffer against the numpy form of the definition"""
    cols, src = fastq_ref.columns(raw)
    assert len(reads) == len(cols["seq_len"]), (ctx, len(reads), len(cols["seq_len"]))
    for attr, name in COLUMNS:
        got = getattr(reads, attr)
        bad = np.flatnonzero(got != cols[name])
        assert not bad.size, (ctx, name, "record", int(bad[0]), "record block", int(bad[0]) // 1024, "raw byte", int(cols["id_start"][int(bad[0])]),
                              int(got[bad[0]]), int(cols[name][bad[0]]))
    assert not (reads.seq_starts % 64).any(), ctx
    assert reads.longest == (int(cols["seq_len"].max()) if len(reads) else 0), ctx
    layout = fastq_ref.layout_np(raw, cols, src)
    assert reads.text_bytes == layout.size and reads.ptr, (ctx, reads.text_bytes, layout.size)
    got = np.frombuffer(reads.download_text(), dtype=np.uint8)
    diff = np.flatnonzero(got != layout)  # sequences, pads, spare bytes
    if diff.size:
        at = int(diff[0])
        rec = int(np.searchsorted(cols["seq_start"], at, side="right")) - 1
        pytest.fail(f"{ctx}: first differing byte {at} of {layout.size} (block {at // 64}), in read {rec} (record block {rec // 1024}), "
                    f"whose sequence starts at raw byte {int(src[rec])} (tile {int(src[rec]) // 4096})")
    return cols


def check(sassy, raw, ctx):
    reads = sassy.DeviceReads(raw)
    try:
        cols = compare(sassy, reads, raw, ctx)
        for i in sorted({0, len(reads) // 2, len(reads) - 1} & set(range(len(reads)))):
            a, n = int(cols["id_start"][i]), int(cols["id_len"][i])
            assert reads.id(i) == bytes(raw[a:a + n]).decode(), (ctx, i)
            a, n = int(cols["qual_start"][i]), int(cols["qual_len"][i])
            assert reads.quality(i) == bytes(raw[a:a + n]), (ctx, i)
            assert reads.text(i).data_ptr() % 64 == 0 and reads.text(i).numel() == int(cols["seq_len"][i]), (ctx, i)
    finally:
        reads.free()
    return cols


# ---------------------------------------------------------------- the parse
def test_the_corpus(sassy):
    for name, raw in fastq_ref.corpus().items():
        check(sassy, raw, name)
        want = fastq_ref.parse(raw)  # the definition itself, line by line
        reads = sassy.DeviceReads(raw)
        assert [reads.download(i) for i in range(len(reads))] == [r.seq for r in want], name
        assert reads.download_text() == fastq_ref.layout(want), name
        reads.free()


def test_read_lengths_around_blocks_tiles_and_super_tiles(sassy):
    rng = random.Random(7)
    lengths = [0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 65537]
    seqs = [bytes(rng.choice(b"ACGTN") for _ in range(n)) for n in lengths]
    for eol in (b"\n", b"\r\n"):
        for order in (seqs, seqs[::-1]):
            for final in (True, False):
                if not final and not order[-1]:
                    continue  # (an empty last quality line exists only with its line end)
                cols = check(sassy, fastq_of(order, eol, final), (eol, final))
                assert cols["seq_len"].tolist() == [len(s) for s in order]


def border_inputs(at):
    """(name, raw): id or sequence padded so that the named line end lands around absolute offset `at`"""
    tail = b"@n x\nACGT\n+\nIIII\n"
    for name, shift, eol in (("newline ends", 1, b"\n"), ("newline begins", 0, b"\n"), ("crlf ends", 2, b"\r\n"), ("crlf across", 1, b"\r\n"),
                             ("crlf begins", 0, b"\r\n")):
        first = at - shift  # where the line end's first byte lies
        yield name + " (id line)", first, b"@" + b"i" * (first - 1) + eol + b"ACG" + eol + b"+" + eol + b"III" + eol + tail
        yield name + " (sequence line)", first, b"@a\n" + b"C" * (first - 3) + eol + b"+\n" + b"I" * 5 + b"\n" + tail
        yield name + " (last line)", first, tail + b"@z\nAC\n+\n" + b"I" * (first - len(tail) - 8) + eol


@pytest.mark.parametrize("at", (64, 4096, 65536))
def test_line_ends_at_the_borders_of_lanes_tiles_and_super_tiles(sassy, at):
    for name, first, raw in border_inputs(at):
        eol = b"\r\n" if "crlf" in name else b"\n"
        assert raw[first:first + len(eol)] == eol, (name, at)
        check(sassy, raw, (name, at))
        if name.endswith("(last line)"):  # and without the final '\n': a last line that ends in '\r', or in a quality byte
            check(sassy, raw[:-1], (name, at, "no final newline"))


def test_a_hundred_thousand_short_reads(sassy):
    """98 blocks of the record scan: block borders, more blocks than a wavefront has lanes, the level above them."""
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 9, size=100_000)
    seqs = [b"ACGTACGT"[:n] for n in lens.tolist()]
    cols = check(sassy, fastq_of(seqs), "100 000 reads")
    assert np.array_equal(cols["seq_len"], lens.astype(np.uint64))


def unit_constants():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "fastq_reads.hip")).read()
    const = lambda name: int(re.search(name + r"\s*=\s*(\d+)", src).group(1))  # noqa: E731
    step = open(os.path.join(ROOT, "sassy_amd", "csrc", "fastq_step.h")).read()
    tile = int(re.search(r"kFqTileBytes\s*=\s*(\d+)", step).group(1))
    threads = {int(x) for x in re.findall(r"__launch_bounds__\((\d+)\) void fastq_(?:scan|rec_top)_kernel", src)}
    assert threads == {1024}
    return tile * const("kTilesPerSuper"), 256 * const("kRecPerThread"), 1024


def test_the_top_level_of_every_scan(sassy):
    """More super-tiles than the scan over them has threads (per = 2) and more record blocks than the scan over those has: the
    sizes come from the unit's constants.  Records of 0 to 8 bases, so that 64 MiB hold more than a million of them; the
    records on both sides of the borders of the top scans' thread runs are long ones, so that their sums differ."""
    super_bytes, rec_block, threads = unit_constants()
    assert (super_bytes, rec_block) == (65536, 1024)
    rng = np.random.default_rng(9)
    kinds = [(b"@%s\n%s\n+\n%s\n" % (b"i" * (n % 3), b"ACGTACGT"[:n], b"IIIIIIII"[:n])) for n in range(9)]
    kinds += [b"@L\r\n" + b"ACGTG" * 13 + b"\r\n+\r\n" + b"I" * 65 + b"\r\n", b"@M\n" + b"TGCAA" * 820 + b"\n+\n" + b"J" * 4100 + b"\n"]
    n_rec = threads * rec_block + rec_block + 6  # 1026 record blocks, the last one of 6 records
    pick = rng.integers(0, 9, size=n_rec)
    for r in (rec_block * 2 - 1, rec_block * 2, threads * rec_block - 1, threads * rec_block, threads * rec_block + 1):
        pick[r] = 9 + r % 2
    raw = b"".join([kinds[k] for k in pick.tolist()])
    if len(raw) <= threads * super_bytes:  # reach 1025 super-tiles whatever the draw
        raw += kinds[10] * ((threads * super_bytes - len(raw)) // len(kinds[10]) + 2)
    assert len(raw) > threads * super_bytes
    raw = np.frombuffer(raw, dtype=np.uint8)
    cols = check(sassy, raw, "top levels")
    assert len(cols["seq_len"]) > threads * rec_block and int(cols["id_start"][threads * rec_block]) > 2 * super_bytes


def test_host_raw_and_device_raw_give_the_same_handle(sassy):
    for raw in (fastq_ref.corpus()["reads.fq"], fastq_ref.corpus()["crlf.fq"][:-2], b"@a\nAC\n+\nII"):
        host = sassy.DeviceReads(raw)
        buf = sassy.DeviceBuffer((len(raw) + 63) // 64 * 64)
        buf.upload(raw)
        dev = sassy.DeviceReads(sassy.DeviceText(buf.ptr, len(raw), owner=buf))
        compare(sassy, dev, raw, "device raw")
        for attr, _ in COLUMNS:
            assert np.array_equal(getattr(host, attr), getattr(dev, attr)), attr
        assert host.download_text() == dev.download_text() and np.array_equal(host.download_rem(), dev.download_rem())
        assert dev.id(len(dev) - 1) == host.id(len(host) - 1) and dev.quality(0) == host.quality(0)
        host.free(), dev.free(), buf.free()
    buf = sassy.DeviceBuffer(64)
    buf.upload(b">a\nAC\n")
    with pytest.raises(sassy.SassyHipError, match="first byte is not '@'"):  # read back before any kernel runs
        sassy.DeviceReads(sassy.DeviceText(buf.ptr, 6, owner=buf))
    buf.free()


def test_malformed_input_names_the_smallest_bad_record(sassy):
    cases = dict(fastq_ref.malformed())
    good = [b"@g%d\n%s\n+\n%s\n" % (i, b"ACGT" * 25, b"I" * 100) for i in range(200)]
    bad_at = 150
    assert len(b"".join(good[:bad_at])) // 4096 >= 7  # the bad record lies in another tile than the first
    cases["no_plus_in_tile_7.fq"] = (b"".join(good[:bad_at]) + good[bad_at].replace(b"\n+\n", b"\nx\n") + b"".join(good[bad_at + 1:]), bad_at, fastq_ref.NO_PLUS)
    cases["no_at_in_tile_7_and_later.fq"] = (b"".join(good[:bad_at]) + b"g" + good[bad_at][1:] + b"".join(good[bad_at + 1:180]) + b"@cut\nAC\n",
                                             bad_at, fastq_ref.NO_AT)
    for name, (raw, record, rule) in cases.items():
        if raw[:1] != b"@":
            with pytest.raises(sassy.SassyHipError, match="first byte is not '@'"):
                sassy.DeviceReads(raw)
            continue
        with pytest.raises(sassy.SassyHipError) as e:
            sassy.DeviceReads(raw)
        assert f"record {record}:" in str(e.value) and rule in str(e.value), (name, str(e.value))
    check(sassy, b"".join(good), "the good records")  # (and the device is fine afterwards)


def test_rem_is_ham_rem_per_block(sassy):
    seqs = [b"", b"", b"ACGT", b"A" * 64, b"", b"", b"", b"C" * 130, b"G" * 65, b"", b"T" * 4097, b"", b""]
    reads = sassy.DeviceReads(fastq_of(seqs))
    want = fastq_ref.rem(reads.seq_starts, reads.seq_lens)
    assert reads.seq_lens.tolist() == [len(s) for s in seqs] and len(want) == (reads.text_bytes - 64) // 64 == 1 + 1 + 3 + 2 + 65
    assert np.array_equal(reads.download_rem(), want)
    assert want[:7].tolist() == [4, 64, 130, 66, 2, 65, 1] and int(reads.seq_starts[-1]) == reads.text_bytes - 64
    reads.free()
    empty = sassy.DeviceReads(fastq_of([b"", b""]))
    assert empty.text_bytes == 64 and empty.download_rem().size == 0 and empty.download_text() == bytes(64)
    empty.free()


# ---------------------------------------------------------------- the three _reads calls
def dna(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(letters) for _ in range(n))


def same_as_many(sassy, s, pats, seqs, k, reads=None, without_trace=False, ctx=None):
    """the three calls over the handle against their siblings over the host list: records field for field, the four
    best-pattern arrays, the counts table"""
    own = reads is None
    reads = sassy.DeviceReads(fastq_of(seqs)) if own else reads
    want = s.search_hamming_many(pats, list(seqs), k, without_trace=without_trace, as_result=True)
    got = s.search_hamming_many(pats, reads, k, without_trace=without_trace, as_result=True)
    assert got.array.dtype == want.array.dtype and len(got.array) == len(want.array), (ctx, len(got.array), len(want.array))
    for field in want.array.dtype.names:
        if field != "cigar_off":
            assert np.array_equal(got.array[field], want.array[field]), (ctx, field)
    assert [x.cigar for x in got.matches] == [x.cigar for x in want.matches], ctx
    if k <= 254:
        for a, b in zip(s.hamming_best_pattern(pats, reads, k), s.hamming_best_pattern(pats, list(seqs), k)):
            assert a.dtype == b.dtype and np.array_equal(a, b), ctx
        assert np.array_equal(s.hamming_counts_many(pats, reads, k), s.hamming_counts_many(pats, list(seqs), k)), ctx
    if own:
        reads.free()
    return want


@functools.lru_cache(maxsize=None)
def read_set(profile, n=300):
    rng = random.Random(21)
    letters = {"dna": b"ACGT", "iupac": b"ACGTACGTNRYKM", "ascii": b"ACGTacgt xyz", "ascii_ci": b"ACGTacgt xyz"}[profile]
    pats = [dna(rng, m) for m in (8, 12, 20, 70, 200)]  # 70 > some reads, 200 > all
    seqs = []
    for i in range(n):
        t = bytearray(dna(rng, rng.choice((0, 1, 7, 30, 63, 64, 65, 100, 150)), letters))
        for p in pats[:3]:
            if len(t) >= len(p) and rng.random() < 0.5:
                at = rng.randrange(len(t) - len(p) + 1)
                w = bytearray(p)
                for _ in range(rng.randrange(3)):
                    w[rng.randrange(len(w))] = rng.choice(letters)
                t[at:at + len(p)] = w
        seqs.append(bytes(t))
    return tuple(pats), tuple(seqs)


@pytest.mark.parametrize("profile,rc", (("dna", True), ("iupac", True), ("ascii", False), ("ascii_ci", False)))
def test_reads_calls_equal_their_many_siblings(sassy, profile, rc):
    pats, seqs = read_set(profile)
    assert any(len(t) < 70 for t in seqs) and all(len(t) < 200 for t in seqs) and len(seqs) > 64
    s = sassy.Searcher(profile, rc=rc)
    reads = sassy.DeviceReads(fastq_of(seqs))
    for k in (0, 2, 20, 300):  # 20 >= m of the short patterns, 300 >= every m: every start is a hit
        want = same_as_many(sassy, s, list(pats), seqs, k, reads=reads, ctx=(profile, k))
        assert len(want.array) > 0 and (k < 20 or len(want.array) > 1000)
    same_as_many(sassy, s, list(pats), seqs, 2, reads=reads, without_trace=True, ctx=(profile, "without trace"))
    # the handle is only read: another searcher takes it too
    s2 = sassy.Searcher(profile, rc=rc)
    same_as_many(sassy, s2, list(pats[:2]), seqs, 1, reads=reads, ctx=(profile, "second searcher"))
    reads.free()
    with pytest.raises(sassy.SassyHipError, match="DeviceReads: freed"):
        s.hamming_best_pattern(list(pats), reads, 1)
    with pytest.raises(sassy.SassyHipError, match="DeviceReads: freed"):
        s.search_hamming_many(list(pats), reads, 1)
    with pytest.raises(sassy.SassyHipError, match="DeviceReads: freed"):
        s.hamming_counts_many(list(pats), reads, 1)


def test_reads_calls_equal_the_references_on_a_small_case(sassy):
    pats, texts, k = cref.HAND_PATTERNS, cref.HAND_TEXTS, cref.HAND_K
    s = sassy.Searcher("dna", rc=True)
    reads = sassy.DeviceReads(fastq_of(texts))
    assert mref.key_matches(s.search_hamming_many(pats, reads, k)) == mref.key_many(mref.expected_many("dna", pats, texts, k, rc=True))
    best = s.hamming_best_pattern(pats, reads, k)
    assert [tuple(int(c[i]) for c in best) for i in range(len(texts))] == mref.expected_best("dna", pats, texts, k, rc=True)
    counts = s.hamming_counts_many(pats, reads, k)
    assert counts.tolist() == cref.HAND_TOTAL and np.array_equal(counts, cref.expected_counts("dna", pats, texts, k, rc=True))
    reads.free()
    rng = random.Random(5)
    pats, seqs = [dna(rng, 6), dna(rng, 9)], [dna(rng, rng.randrange(0, 90)) for _ in range(40)]
    reads = sassy.DeviceReads(fastq_of(seqs, b"\r\n"))
    s = sassy.Searcher("iupac", rc=True).with_max_n_frac(0.2)
    assert mref.key_matches(s.search_hamming_many(pats, reads, 2)) == \
        mref.key_many(mref.expected_many("iupac", pats, seqs, 2, rc=True, max_n_frac=0.2))
    assert np.array_equal(s.hamming_counts_many(pats, reads, 2), cref.expected_counts("iupac", pats, seqs, 2, rc=True, max_n_frac=0.2))
    reads.free()


def test_a_live_decoy_across_a_reads_end(sassy):
    """A window that runs across a read's end into the pad, and one that runs into the next read: on the laid-out buffer both
    are hits, in the batch they are none."""
    pattern = b"ACGGTCATTGCAAGCT"
    half = len(pattern) // 2
    seqs = []
    for j in (1, 2, 64):  # a read of exactly 64 j bytes ends in the first half, the next begins with the second
        seqs.append((b"AC" * (32 * j))[:64 * j - half] + pattern[:half])
        seqs.append(pattern[half:] + b"CA" * 11)
    pats = [pattern]
    for letter in b"ACGT":  # 62 bytes ending in four of a letter: the pattern of six reaches two bytes into the padding
        other = bytes(c for c in b"ACGT" if (c >> 1) & 3 != (letter >> 1) & 3)
        seqs.append((other * 20)[:58] + bytes([letter]) * 4)
        pats.append(bytes([letter]) * 6)
    s = sassy.Searcher("dna", rc=False)
    reads = sassy.DeviceReads(fastq_of(seqs))
    assert s.search_hamming_many(pats, reads, 0) == [] and mref.expected_many("dna", pats, seqs, 0) == []
    assert set(s.hamming_best_pattern(pats, reads, 0)[0].tolist()) == {mref.NO_MATCH} and not s.hamming_counts_many(pats, reads, 0).any()
    s = sassy.Searcher("dna", rc=True)
    want = same_as_many(sassy, s, pats, seqs, 2, reads=reads, ctx="decoys, k = 2")
    assert mref.key_matches(want.matches) == mref.key_many(mref.expected_many("dna", pats, seqs, 2, rc=True))
    reads.free()


def test_seams_of_pattern_groups_and_ranges(sassy):
    pats, seqs = read_set("dna")
    seqs = seqs * 3  # 900 reads: 15 tiles of blocks and more
    s = sassy.Searcher("dna", rc=True)
    s.set_option("hamming_items", 64).set_option("hamming_batch", 1).set_option("hamming_records", 100)
    plain = sassy.Searcher("dna", rc=True)
    reads = sassy.DeviceReads(fastq_of(seqs))
    for k in (1, 3):
        want = same_as_many(sassy, s, list(pats), seqs, k, reads=reads, ctx=("seams", k))
        s.search_hamming_many(list(pats), reads, k)
        got = plain.search_hamming_many(list(pats), reads, k, as_result=True)
        assert np.array_equal(got.array["text_start"], want.array["text_start"]) and np.array_equal(got.array["text_idx"], want.array["text_idx"])
        assert s.stats()["scan_launches"] > plain.stats()["scan_launches"]  # one pattern per group, ranges cut by the item list
    reads.free()


def test_max_n_frac(sassy):
    rng = random.Random(31)
    pats = [dna(rng, 10), dna(rng, 16)]
    seqs = []
    for i in range(200):  # one N in thirteen bytes, and the first pattern planted with 0 .. 2 of its bytes made N
        t = bytearray(dna(rng, rng.randrange(0, 120), b"ACGTACGTACGTN"))
        if len(t) >= 30:
            w = bytearray(pats[0])
            for at in rng.sample(range(10), i % 3):
                w[at] = ord("N")
            t[7:17] = w
        seqs.append(bytes(t))
    found = []
    for frac in (0.0, 0.1, 0.5):
        s = sassy.Searcher("iupac", rc=True).with_max_n_frac(frac)
        found.append(len(same_as_many(sassy, s, pats, seqs, 3, ctx=("max_n_frac", frac)).array))
    assert 0 < found[0] < found[1] < found[2], found  # the rule drops hits, and fewer of them as it loosens


# ---------------------------------------------------------------- the reader and the CLI
def test_reader_and_cli_write_the_same_bytes(sassy, tmp_path, monkeypatch):
    from sassy_amd import cli, fastx
    rng = random.Random(41)
    barcodes = [dna(rng, 12) for _ in range(8)]
    seqs = []
    for i in range(400):
        t = bytearray(dna(rng, rng.choice((0, 20, 80, 150))))
        if len(t) >= 12 and i % 5:
            t[3:15] = barcodes[i % 8]
            t[5] = ord("A")
        seqs.append(bytes(t))
    raw = fastq_of(seqs, b"\n")
    plain, gz = tmp_path / "reads.fq", tmp_path / "reads.fq.gz"
    plain.write_bytes(raw)
    gz.write_bytes(gzip.compress(raw))
    pat_file = tmp_path / "barcodes.txt"
    pat_file.write_bytes(b"\n".join(barcodes) + b"\n")
    monkeypatch.setattr(cli, "BATCH_BYTES", 9000)  # several chunks
    host = [(rb.id(i), rb.sequence(i)) for rb in fastx.read_fastx_batches(str(plain), 9000) for i in range(len(rb))]
    batches = 0
    for path in (plain, gz):
        got = []
        for batch in fastx.read_fastq_device_batches(str(path), 9000):
            got += [(batch.id(i), batch.sequence(i)) for i in range(len(batch))]
            batch.free()
            batches += 1
        assert got == host and len(got) == len(seqs), path
    assert batches >= 8

    def run(argv):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            assert cli.main(argv) == 0
        return out.getvalue()
    for path in (plain, gz):
        demux = ["demux", "-l", str(pat_file), "-k", "2", str(path)]
        a, b = run(demux), run(demux + ["--device-parse"])
        assert a == b and a.count("\n") == len(seqs) + 1 and "\t+\t" in a, path
        count = ["count", str(pat_file), str(path), "-k", "2", "--rc", "-a", "dna"]
        a, b = run(count), run(count + ["--device-parse"])
        assert a == b and a.count("\n") == 1 + 2 * len(barcodes), path
