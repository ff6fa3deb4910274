"""FASTA unwrap on the device (sassy_amd/csrc/fasta_unwrap.hip) against the line-by-line parse (tests/helpers/fasta_ref.py).

Every case compares the whole result: ids, lengths, starts (multiples of 64) and the device buffer byte for byte -- every
record's sequence, the zero pads between them and the 64 spare bytes -- which is what fasta_ref.layout builds.  Inputs are a
few MB each, but for the three that exist for their size (tests/helpers/scan_levels.py: two of 64 MiB, one of a million
records).  Geometry the shapes aim at: 64 bytes per lane, 4 KiB per tile (a wavefront), 64 KiB per super-tile (a workgroup of
the count pass); the record scan works in blocks of 1 024 records under one workgroup of 1 024 threads, so 70 000 records are
69 blocks: block borders, more blocks than a wavefront has lanes, and the level above them.  The upper levels: the scan of the
super-tile summaries is one workgroup of 1 024 threads, each folding `per` = ceil(n_super / 1024) summaries in order -- 1 025
super-tiles make per = 2; the compact pass runs at most 4 096 workgroups of one tile at a time -- 16 386 tiles make a
workgroup reuse its LDS images; the scan of the record block sums gives each of 1 024 threads `per` blocks -- 1 026 blocks
make per = 2.  Not reached: the record pass's grid cap of 2^20 workgroups (more than 16 GiB of input)."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import fasta_ref  # noqa: E402
import scan_levels as lv  # noqa: E402

pytestmark = pytest.mark.gpu

BORDERS = (63, 64, 4095, 4096, 65535, 65536)


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


def first_diff(a: bytes, b: bytes) -> int:
    n = min(len(a), len(b))
    x = np.flatnonzero(np.frombuffer(a, np.uint8, n) != np.frombuffer(b, np.uint8, n))
    return int(x[0]) if x.size else n


def columns(want):
    return {"id_starts": [r.id_start for r in want], "id_lens": [r.id_len for r in want],
            "seq_starts": [r.seq_start for r in want], "seq_lens": [r.seq_len for r in want]}


def compare_with(sassy, fa, cols, layout: bytes, ctx):
    """the table, column by column, and the whole device buffer; a mismatch names the record, its block of the record scan
    and the super-tile its '>' lies in"""
    n_rec = len(cols["id_starts"])
    assert len(fa) == n_rec, (ctx, len(fa), n_rec)
    for name in ("id_starts", "id_lens", "seq_starts", "seq_lens"):
        got, col = getattr(fa, name), np.asarray(cols[name], dtype=np.uint64)
        bad = np.flatnonzero(got != col)
        assert not bad.size, (ctx, name, "record", int(bad[0]), "record block", int(bad[0]) // 1024, "super-tile",
                              int(cols["id_starts"][int(bad[0])]) // 65536, int(got[bad[0]]), int(col[bad[0]]))
    assert not (fa.seq_starts % 64).any(), ctx
    assert fa.text_bytes == len(layout) and fa.ptr, (ctx, fa.text_bytes, len(layout))
    got = sassy.DeviceText(fa.ptr, fa.text_bytes).download()
    if got != layout:  # sequences, pads, spare bytes
        at = first_diff(got, layout)
        rec = int(np.searchsorted(np.asarray(cols["seq_starts"], dtype=np.uint64), at, side="right")) - 1
        raw_at = int(cols["id_starts"][rec]) + int(cols["id_lens"][rec]) + at - int(cols["seq_starts"][rec])  # (but for line ends)
        pytest.fail(f"{ctx}: first differing byte {at} of {len(layout)}, in record {rec} (record block {rec // 1024}), near raw byte "
                    f"{raw_at} (tile {raw_at // 4096}, super-tile {raw_at // 65536})")


def compare(sassy, fa, raw: bytes, ctx, want=None, layout=None):
    want = fasta_ref.parse(raw) if want is None else want
    compare_with(sassy, fa, columns(want), fasta_ref.layout(want) if layout is None else layout, ctx)
    for i in sorted(set(list(range(min(3, len(want)))) + list(range(max(0, len(want) - 3), len(want))))):
        assert fa.download(i) == want[i].seq and fa.text(i).numel() == len(want[i].seq), (ctx, i)
        assert fa.text(i).data_ptr() % 64 == 0, (ctx, i)
    return want


def check(sassy, raw: bytes, ctx):
    fa = sassy.DeviceFasta(raw)
    try:
        want = compare(sassy, fa, raw, ctx)
        for i in (0, len(want) - 1):
            if want:
                assert fa.id(i) == raw[want[i].id_start:want[i].id_start + want[i].id_len].decode(), (ctx, i)
    finally:
        fa.free()
    return want


def test_small_inputs(sassy):
    for raw in (b"", b">", b">a\nACGT", b">a\nACGT\n", b">\n", b">a\r", b">a\r\n", b">a\nA", b">a\n\r", b">a\n\n", b">a\n>b\n>c"):
        want = check(sassy, raw, raw)
    assert [r.seq for r in check(sassy, b">a\nACGT", "hand")] == [b"ACGT"]
    assert check(sassy, b"", "empty") == []


def border_inputs(at: int):
    """(name, raw): the first id is padded so that the named byte lands at absolute offset `at`."""
    pad = lambda k: b"i" * k  # noqa: E731
    yield "header >", b">" + pad(at - 5) + b"\nAC\n" + b">next d\nACGT\nGG\n"
    yield "header newline", b">" + pad(at - 1) + b"\nACGT\nGG\n>n\nT\n"
    yield "header crlf", b">" + pad(at - 2) + b"\r\nACGT\r\nGG\r\n"
    yield "sequence newline", b">" + pad(at - 7) + b"\nACGTA\nGG\nT\n"
    yield "crlf across", b">" + pad(at - 7) + b"\nACGT\r\nGG\r\nT\r\n"
    yield "last byte cr", b">" + pad(at - 4) + b"\nAC\r"
    yield "last byte newline", b">" + pad(at - 4) + b"\nAC\n"
    yield "last byte base", b">" + pad(at - 4) + b"\nACG"
    yield "last byte in header", b">" + pad(at - 6) + b"\nAC\n>x"
    yield "last byte header >", b">" + pad(at - 5) + b"\nAC\n>"
    yield "last byte header cr", b">" + pad(at - 7) + b"\nAC\n>x\r"


@pytest.mark.parametrize("at", BORDERS)
def test_borders_of_lanes_tiles_and_super_tiles(sassy, at):
    for name, raw in border_inputs(at):
        if name == "header >":
            assert raw[at:at + 1] == b">" and raw[at - 1:at] == b"\n"
        elif name in ("header newline", "sequence newline"):
            assert raw[at:at + 1] == b"\n" and raw[at - 1:at] != b"\r"
        elif name in ("crlf across", "header crlf"):
            assert raw[at - 1:at + 1] == b"\r\n"
        else:
            assert len(raw) == at + 1, (name, len(raw))
        check(sassy, raw, (name, at))


def wrapped(seq: bytes, width: int, eol: bytes = b"\n") -> bytes:
    return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def dna(rng, n: int) -> bytes:
    return bytes(rng.choice(b"ACGTNacgt") for _ in range(n))


def test_line_widths(sassy):
    rng = random.Random(11)
    every = b""
    for w in (1, 59, 60, 63, 64, 65, 70, 4095, 4096, 4097):
        n = 3 * w + w // 2 + 1 if w > 1 else 150
        raw = b">w%d\n" % w + wrapped(dna(rng, n), w) + b">crlf%d x\r\n" % w + wrapped(dna(rng, 2 * w + 1), w, b"\r\n")
        check(sassy, raw, ("width", w))
        every += raw
    every += b">one line\n" + dna(rng, 10000)  # no newline behind it
    check(sassy, every, "all widths, then 10 000 bytes without a newline")


def test_long_headers_carry_the_state_through_tiles(sassy):
    rng = random.Random(12)
    raw = b">" + b"h" * 5000 + b"\nACGT\nGG\n>" + b"H>" * 35000 + b"\n" + wrapped(dna(rng, 700), 60) + b">t\nT\n"
    check(sassy, raw, "headers of 5 000 and 70 000 bytes")
    check(sassy, raw + b">" + b"e" * 70000, "a 70 000-byte header ends the input")
    check(sassy, raw + b">" + b"e" * 70000 + b"\r", "... with a carriage return")
    check(sassy, b">" + b"x" * (65536 * 2 + 17) + b"\r\nAC\n", "a header through two super-tiles")


def test_gt_that_begins_no_line(sassy):
    rng = random.Random(13)
    check(sassy, b">a>b >c\nAC>GT\n>\n>>\nA>\n>d\n>>>\n", "> inside headers and sequence lines")
    for tile in (4096, 65536):
        body = b">r\n" + wrapped(dna(rng, tile), 61)
        for prev in (b"A", b"\n", b"\r"):
            raw = body[:tile - 1] + prev + b">x y\nACGT\nGG\n"
            assert raw[tile:tile + 1] == b">" and raw[tile - 1:tile] == prev
            want = check(sassy, raw, ("> as a tile's first byte behind", prev, tile))
            assert len(want) == (2 if prev == b"\n" else 1)


def test_empty_records_and_blank_lines(sassy):
    rng = random.Random(14)
    check(sassy, b">first\n>b\nAC\n>c\n>d\n>e\nGG\n>last\n", "empty records first, last and in runs")
    check(sassy, b">a\n\n\nAC\n\nGT\n\n>b\n\n>c\n\r\n\r\nT\r\n\n", "blank lines")
    check(sassy, b">a\nAC\n>last without newline", "a header as the last line")
    for lead in (63, 64, 4096 - 3, 4096 + 64 - 3):  # 32 headers of two bytes: inside one lane, and across two
        raw = b">" + b"i" * (lead - 2) + b"\n" + b">\n" * 32 + b">z\nACGT\n"
        check(sassy, raw, ("32 empty records from offset", lead))
    raw = b"".join(b">%d\n" % i + (wrapped(dna(rng, rng.randrange(1, 130)), 60) if rng.random() < 0.5 else b"") for i in range(3000))
    check(sassy, raw, "3 000 records, half of them empty")


def test_alignment_and_padding_of_neighbouring_records(sassy):
    rng = random.Random(15)
    lens = [0, 1, 63, 64, 65, 4096, 0, 0, 65, 64, 63, 1, 0, 4096, 4097, 127, 128, 129]
    raw = b"".join(b">len%d\n" % n + wrapped(dna(rng, n), 60) for n in lens)
    want = check(sassy, raw, "record lengths 0, 1, 63, 64, 65, 4096 next to each other")
    assert [r.seq_len for r in want] == lens


def test_many_records_cross_the_record_scans_blocks(sassy):
    want = check(sassy, b">a\nA\n" * 70000, "70 000 records")
    assert len(want) == 70000 and want[-1].seq_start == 64 * 69999


@pytest.mark.parametrize("variant", (0, 1))
def test_more_than_1024_super_tiles(sassy, variant):
    """64 MiB + 5000 bytes (scan_levels.fasta_big): n_super = 1025, so every thread of fasta_scan_kernel folds per = 2
    super-tile summaries (thread 512 one, the threads behind it none), and n_tiles = 16 386 on 4096 workgroups of
    fasta_compact_kernel, up to 5 tiles each.  Once from host bytes, once from a device-resident buffer."""
    arr, at = lv.fasta_big(variant)
    raw = arr.tobytes()
    want = fasta_ref.parse(raw)
    layout = fasta_ref.layout(want)
    n_super, n_tiles = -(-len(raw) // lv.SUPER), -(-len(raw) // lv.TILE)
    print(f"variant {variant}: {len(raw)} bytes, n_super={n_super} per={-(-n_super // 1024)} n_tiles={n_tiles} "
          f"tiles of workgroup 0={len(range(0, n_tiles, 4096))} records={len(want)}")
    assert n_super == 1025 and len(range(0, n_tiles, 4096)) == 5
    host = sassy.DeviceFasta(raw)
    try:
        compare(sassy, host, raw, ("host", variant), want, layout)
    finally:
        host.free()
    buf = sassy.DeviceBuffer((len(raw) + 63) // 64 * 64)
    buf.upload(raw)
    dev = sassy.DeviceFasta(sassy.DeviceText(buf.ptr, len(raw), owner=buf))
    try:
        compare(sassy, dev, raw, ("device", variant), want, layout)
    finally:
        dev.free()
        buf.free()


def test_more_than_1024_record_blocks(sassy):
    """1 048 576 + 1030 records (scan_levels.fasta_many_records): n_blocks = 1026 blocks of the record scan, so
    fasta_rec_top_kernel runs with per = 2 -- thread 512 owns the last full block and the one of 6 records, the threads
    behind it nothing.  The expectation is the closed form, which test_scan_levels_cpu compares with the line-by-line parse
    around every planted border."""
    raw, cols, layout = lv.fasta_many_records()
    n_blocks = -(-lv.FASTA_MANY_RECORDS // lv.REC_BLOCK)
    print(f"{len(raw)} bytes, records={lv.FASTA_MANY_RECORDS} n_blocks={n_blocks} per={-(-n_blocks // 1024)} layout={len(layout)}")
    assert n_blocks == 1026
    fa = sassy.DeviceFasta(raw)
    try:
        compare_with(sassy, fa, cols, layout, "1 049 606 records")
        for r in (0, 1023 * 1024 + 1, 1024 * 1024 - 1, lv.FASTA_MANY_RECORDS - 1):
            a, n = int(cols["seq_starts"][r]), int(cols["seq_lens"][r])
            assert fa.download(r) == layout[a:a + n] and fa.text(r).data_ptr() % 64 == 0, r
    finally:
        fa.free()


def test_host_and_device_resident_input_agree(sassy):
    rng = random.Random(16)
    raw = b"".join(b">chr%d desc\r\n" % i + wrapped(dna(rng, n), 60, b"\r\n" if i % 2 else b"\n") for i, n in enumerate([5000, 0, 61, 70000, 4096]))
    for cut in (len(raw), len(raw) - 1, 4096 * 3 + 1):  # (a cut inside a line: still whole records by the definition)
        data = raw[:cut]
        host = sassy.DeviceFasta(data)
        buf = sassy.DeviceBuffer((len(data) + 63) // 64 * 64)
        buf.upload(data)
        dev = sassy.DeviceFasta(sassy.DeviceText(buf.ptr, len(data), owner=buf))
        try:
            want = compare(sassy, host, data, ("host", cut))
            compare(sassy, dev, data, ("device", cut))
            for name in ("id_starts", "id_lens", "seq_starts", "seq_lens"):
                assert (getattr(host, name) == getattr(dev, name)).all(), (name, cut)
            assert sassy.DeviceText(host.ptr, host.text_bytes).download() == sassy.DeviceText(dev.ptr, dev.text_bytes).download()
            assert [dev.id(i) for i in range(len(dev))] == [host.id(i) for i in range(len(host))] == \
                [data[r.id_start:r.id_start + r.id_len].decode() for r in want]
        finally:
            host.free()
            dev.free()
            buf.free()
    with pytest.raises(sassy.SassyHipError, match="first byte is not '>'"):
        buf = sassy.DeviceBuffer(64)
        buf.upload(b"ACGT\n" + bytes(59))
        sassy.DeviceFasta(sassy.DeviceText(buf.ptr, 5, owner=buf))


def random_file(rng) -> bytes:
    if rng.random() < 0.3:  # raw noise over the four bytes that matter
        special = rng.choice((1, 4, 16, 64))
        body = bytes(rng.choice(b"\n\r>") if rng.randrange(64) < special else 65 for _ in range(rng.randrange(1, 9000)))
        return b">" + body
    out = []
    for r in range(rng.randrange(1, 12)):
        out.append(b">" + bytes(rng.choice(b"ab >\r1") for _ in range(rng.randrange(0, 80))))
        out.append(rng.choice((b"\n", b"\r\n")))
        width = rng.choice((1, 7, 60, 63, 64, 65, 80, 500))
        seq = bytes(rng.choice(b"ACGTN>\r") if rng.random() < 0.05 else rng.choice(b"ACGT") for _ in range(rng.choice((0, 1, 59, 64, 300, 5000))))
        for i in range(0, len(seq), width):
            out.append(seq[i:i + width] + rng.choice((b"\n", b"\r\n")))
            if rng.random() < 0.05:
                out.append(rng.choice((b"\n", b"\r\n")))
    raw = b"".join(out)
    cut = rng.choice((0, 0, 1, 2))
    return raw[:len(raw) - cut] if cut and len(raw) > cut + 1 else raw


def test_random_small_files_with_mixed_line_ends(sassy):
    rng = random.Random(20261019)
    for i in range(300):
        check(sassy, random_file(rng), ("random file", i))


# ---------------------------------------------------------------- end to end: the views are texts
def revcomp(s: bytes) -> bytes:
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


@pytest.fixture(scope="module")
def planted():
    """Three records: an empty one, one shorter than the pattern, one of a few tiles with planted hits and a product."""
    rng = random.Random(17)
    pat = bytes(rng.choice(b"ACGT") for _ in range(24))
    fwd, rev = bytes(rng.choice(b"ACGT") for _ in range(20)), bytes(rng.choice(b"ACGT") for _ in range(22))
    long = bytearray(rng.choice(b"ACGT") for _ in range(3 * 4096 + 100))
    for at, edits in ((100, 0), (4090, 1), (8192 - 12, 2), (3 * 4096 + 100 - 24, 0)):
        hit = bytearray(pat)
        for e in range(edits):
            hit[3 + 7 * e] = ord("A") if hit[3 + 7 * e] != ord("A") else ord("C")
        long[at:at + 24] = hit
    long[5000:5020] = fwd
    long[5300:5322] = revcomp(rev)
    long[9000:9022] = rev  # strand '-': rev on the forward strand, reverse_complement(fwd) behind it
    long[9400:9420] = revcomp(fwd)
    raw = b">empty\n>short one\r\nACGTAC\r\n>long\n" + wrapped(bytes(long), 60)
    return raw, pat, (fwd, rev)


def test_views_search_like_host_texts(sassy, planted):
    raw, pat, pair = planted
    ref = fasta_ref.parse(raw)
    fa = sassy.DeviceFasta(raw)
    try:
        assert [len(r.seq) for r in ref] == [0, 6, 3 * 4096 + 100]
        key = lambda ms: [(m.pattern_idx, m.text_start, m.text_end, m.cost, m.strand, m.cigar) for m in ms]  # noqa: E731
        found = 0
        for i, r in enumerate(ref):
            s = sassy.Searcher("dna", rc=True)
            got, want = s.search(pat, fa.text(i), 2), s.search(pat, r.seq, 2)
            assert key(got) == key(want), ("search", i)
            found += len(got)
            got, want = s.search_hamming([pat, pat[:12]], fa.text(i), 2), s.search_hamming([pat, pat[:12]], r.seq, 2)
            assert key(got) == key(want), ("search_hamming", i)
            assert (s.hamming_counts([pat, pat[:12]], fa.text(i), 2) == s.hamming_counts([pat, pat[:12]], r.seq, 2)).all(), ("hamming_counts", i)
            got, want = s.hamming_amplicons([pair], fa.text(i), 1, 50, 1000), s.hamming_amplicons([pair], r.seq, 1, 50, 1000)
            assert got.tobytes() == want.tobytes() and len(got) == (2 if i == 2 else 0), ("hamming_amplicons", i, len(got))
        assert found >= 4
    finally:
        fa.free()


def test_cli_writes_the_same_bytes_with_device_unwrap(sassy, planted, tmp_path, capsys):
    from sassy_amd import cli, fastx
    raw, pat, (fwd, rev) = planted
    fasta, primers, pats = tmp_path / "g.fa", tmp_path / "p.tsv", tmp_path / "pats.txt"
    fasta.write_bytes(raw + b">tail\r\nGG\r\n")
    primers.write_bytes(b"pair1\t" + fwd + b"\t" + rev + b"\n")
    pats.write_bytes(pat + b"\n" + pat[:12] + b"\n")
    batches = list(fastx.read_fasta_device_batches(str(fasta), 64))  # (batches smaller than a record)
    assert [(b.id(i), b.sequence(i)) for b in batches for i in range(len(b))] == fasta_ref.ids_and_sequences(raw + b">tail\r\nGG\r\n")
    assert len(batches) >= 2 and batches[-1].text(0).is_cuda  # (the long record and what follows it: one batch)

    def run(argv):
        capsys.readouterr()
        assert cli.main(argv) == 0
        return capsys.readouterr().out
    for argv in (["amplicon", str(primers), str(fasta), "-k", "1", "--min-len", "50", "--max-len", "1000", "-a", "dna"],
                 ["amplicon", str(primers), str(fasta), "-k", "1", "--min-len", "50", "--max-len", "1000", "-a", "dna", "--seq"],
                 ["count", str(pats), str(fasta), "-k", "2", "--rc", "-a", "dna", "--per-record"]):
        plain, device = run(argv), run(argv + ["--device-unwrap"])
        assert plain == device and plain.count("\n") >= 3, argv
