"""Searcher.best_matches on the GPU (sassy_hip_best_matches, `python -m sassy_amd search --best`) against the CPU oracle:
the expected records come from the oracle's matches of every (pattern, text) pair by the definition in
include/sassy_hip.h (tests/helpers/best_matches_ref.py).  Exact equality, record by record including the cigars; every
case with best_match_device 1 (the locating reduction and one traceback per text, where a one-pass batch path takes the
call) and 0 (search_many's records reduced by the host); (cost, pattern, strand) must equal best_pattern's arrays."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import best_matches_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NO = 255


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    assert sassy_amd.device_count() > 0, "no HIP device: the GPU tests must not silently skip"
    return sassy_amd


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, edits, alphabet=b"ACGT"):
    s = bytearray(s)
    for _ in range(edits):
        t, p = rng.randrange(3), rng.randrange(len(s))
        if t == 0:
            s[p] = rng.choice(alphabet)
        elif t == 1:
            s.insert(p, rng.choice(alphabet))
        elif len(s) > 1:
            del s[p]
    return bytes(s)


def check(s, pats, texts, k, want, ctx, device_stats=None, host_texts=None, best_pattern=True):
    """Both paths, exactly the expected records.  device_stats: the `filtered` codes the device run must show (5 tiled
    scan, 6 seeded search) -- the one-pass path took the call -- and at timing level 2 trace_ms > 0: the reduction ran."""
    n_texts = len(host_texts if host_texts is not None else texts)
    if device_stats:
        s.set_timing(2)
    for dev in (1, 0):
        s.set_option("best_match_device", dev)
        try:
            ms = s.best_matches(pats, texts, k)
            st = s.stats()
            got = [ref.got_record(m) for m in ms]
            bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
            print(ctx, "dev", dev, "records", len(got), "expected", len(want), "mismatches", len(bad))
            assert len(got) == len(want), (ctx, dev, len(got), len(want))
            assert not bad, (ctx, dev, bad[:5], [got[i] for i in bad[:3]], [want[i] for i in bad[:3]])
            assert [g[0] for g in got] == sorted(g[0] for g in got)
            if device_stats and dev:
                assert st["filtered"] in device_stats and st["candidates"] > 0 and st["trace_ms"] > 0, (ctx, dev, st)
            wt = [ref.got_record(m) for m in s.best_matches(pats, texts, k, without_trace=True)]
            assert wt == [ref.without_trace(w) for w in want], (ctx, dev, "without trace", wt[:3], want[:3])
            arr = s.best_matches(pats, texts, k, as_result=True).array
            assert len(arr) == len(want)
            if best_pattern:
                c, p, sd = s.best_pattern(pats, texts, k)
                bc, bp, bs = np.full(n_texts, NO, np.uint8), np.full(n_texts, 0xFFFFFFFF, np.uint32), np.zeros(n_texts, np.uint8)
                ti = arr["text_idx"].astype(np.int64)
                bc[ti], bp[ti], bs[ti] = arr["cost"], arr["pattern_idx"], arr["strand"]
                assert np.array_equal(c, bc) and np.array_equal(p, bp) and np.array_equal(sd, bs), (ctx, dev, "best_pattern")
        finally:
            s.set_option("best_match_device", 1)


def barcode_reads(rng, pats, n_reads, k, lo, hi, profile="iupac"):
    """Reads with a planted barcode at 0 .. k edits (either strand, anywhere, the two ends included) and reads without."""
    reads = []
    for i in range(n_reads):
        n = rng.randrange(lo, hi)
        tx = bytearray(rand_seq(rng, n))
        if i % 5 != 4:
            ins = mutate(rng, rng.choice(pats), rng.randrange(0, k + 1))
            if rng.random() < 0.5:
                ins = oracle.reverse_complement(profile, ins)
            at = rng.choice([0, n - len(ins), rng.randrange(0, n - len(ins) + 1)])
            tx[at:at + len(ins)] = ins
        reads.append(bytes(tx))
    return reads


def test_barcodes_over_reads_device_path(sassy):
    """96 x 24 bp over 20 000 reads of 200 - 1 000 bp with planted mutated barcodes, k = 3, Iupac, both strands; the seeded
    search and the tiled scan forced in turn."""
    rng = random.Random(4242)
    pats = [rand_seq(rng, 24) for _ in range(96)]
    reads = barcode_reads(rng, pats, 20000, 3, 200, 1001)
    want = ref.expected_fast("iupac", pats, reads, 3, True)
    assert len(want) >= 15000 and sum(1 for w in want if w[7] == "-") >= 5000
    for mode, code in (("seeded", 6), ("tiled", 5)):
        s = sassy.Searcher("iupac", rc=True)
        s.set_option("many_tiled", 1)
        s.set_option("many_seeded", 1 if mode == "seeded" else 0)
        check(s, pats, reads, 3, want, ("barcodes", mode), device_stats=(code,))
    # the searcher's own only_best_match setting does not change the answer
    s = sassy.Searcher("iupac", rc=True).only_best_match()
    assert [ref.got_record(m) for m in s.best_matches(pats, reads[:3000], 3)] == [w for w in want if w[0] < 3000]


def test_forward_only_dna(sassy):
    rng = random.Random(5)
    pats = [rand_seq(rng, 20) for _ in range(40)]
    reads = barcode_reads(rng, pats, 1500, 2, 100, 600, "dna")
    want = ref.expected_fast("dna", pats, reads, 2, False)
    assert len(want) >= 500 and all(w[7] == "+" for w in want)
    for seeded in (1, 0):
        s = sassy.Searcher("dna", rc=False)
        s.set_option("many_tiled", 1)
        s.set_option("many_seeded", seeded)
        check(s, pats, reads, 2, want, ("dna fwd", seeded), device_stats=(5, 6))


def test_overhang_over_either_end(sassy):
    """alpha = 0.5: barcodes hanging over the front and the back of the read (cut off there), inside it, and none."""
    rng = random.Random(6)
    alpha, k = 0.5, 3
    pats = [rand_seq(rng, 24) for _ in range(12)]
    texts = []
    for i in range(400):
        n = rng.randrange(40, 300)
        tx = bytearray(rand_seq(rng, n))
        ins = mutate(rng, pats[i % 12], i % 3)
        if (i // 4) % 2:
            ins = oracle.reverse_complement("iupac", ins)
        cut = rng.randrange(1, 7)
        where = i % 4
        if where == 0:
            tx[0:len(ins) - cut] = ins[cut:]
        elif where == 1:
            tx[n - (len(ins) - cut):] = ins[:len(ins) - cut]
        elif where == 2:
            at = rng.randrange(0, n - len(ins))
            tx[at:at + len(ins)] = ins
        texts.append(bytes(tx))
    texts[7] = b""
    for rc in (True, False):
        want = ref.expected(lambda p, t: oracle.search_overhang("iupac", p, t, k, alpha, rc=rc), pats, texts)
        assert sum(1 for w in want if w[5] < 24) >= 30 and sum(1 for w in want if w[4] > 0) >= 30  # hang over the back / the front
        for tiled, seeded in ((1, 1), (1, 0), (0, 0)):
            s = sassy.Searcher("iupac", rc=rc, alpha=alpha)
            s.set_option("overhang_tiled", tiled)
            s.set_option("overhang_seeded", seeded)
            check(s, pats, texts, k, want, ("overhang", rc, tiled, seeded), device_stats=(5, 6) if tiled else None)


def test_nothing_matches_and_empty_texts(sassy):
    rng = random.Random(7)
    pats = [rand_seq(rng, 24) for _ in range(8)]
    texts = [b"", rand_seq(rng, 300), b"", b"ACG", rand_seq(rng, 24), b""]
    for k in (0, 1):
        want = ref.expected(lambda p, t: oracle.search("iupac", p, t, k, rc=True), pats, texts)
        assert want == []
        s = sassy.Searcher("iupac", rc=True)
        s.set_option("many_tiled", 1)
        check(s, pats, texts, k, want, ("nothing", k))
    # ... and the same texts around two that do match
    texts2 = texts[:3] + [rand_seq(rng, 50) + pats[3] + rand_seq(rng, 9)] + texts[3:] + [oracle.reverse_complement("iupac", pats[5])]
    want = ref.expected(lambda p, t: oracle.search("iupac", p, t, 1, rc=True), pats, texts2)
    assert [(w[0], w[1], w[7]) for w in want] == [(3, 3, "+"), (7, 5, "-")]
    for tiled in (1, -1):
        s = sassy.Searcher("iupac", rc=True)
        s.set_option("many_tiled", tiled)
        check(s, pats, texts2, 1, want, ("nothing but two", tiled))
    assert sassy.Searcher("iupac", rc=True).best_matches(pats, [], 1) == []
    assert sassy.Searcher("iupac", rc=True).best_matches([], texts, 1) == []


def test_ties(sassy):
    """The same barcode twice in a read at equal cost (on each strand): the rightmost in scan direction; two barcodes at
    equal cost: the lower index; a palindromic hit on both strands: Fwd."""
    rng = random.Random(8)
    half = rand_seq(rng, 12)
    palin = half + oracle.reverse_complement("iupac", half)
    assert oracle.reverse_complement("iupac", palin) == palin
    pats = [rand_seq(rng, 24) for _ in range(8)]
    pats[5] = pats[2]
    pats[6] = palin
    reads = []
    for i in range(320):
        which = [pats[2], pats[1], palin, pats[7]][i % 4]
        edits = (i // 4) % 3
        occ = mutate(rng, which, edits)
        kind = (i // 12) % 4
        if kind == 0:      # twice, forward
            tx = rand_seq(rng, 30) + occ + rand_seq(rng, rng.randrange(1, 60)) + occ + rand_seq(rng, 20)
        elif kind == 1:    # twice, reverse complement
            r = oracle.reverse_complement("iupac", occ)
            tx = rand_seq(rng, 30) + r + rand_seq(rng, rng.randrange(1, 60)) + r + rand_seq(rng, 20)
        elif kind == 2:    # two barcodes at the same number of edits, the second on the other strand
            other = oracle.reverse_complement("iupac", mutate(rng, pats[0], edits))
            tx = rand_seq(rng, 10) + occ + rand_seq(rng, 40) + other
        else:              # once on each strand
            tx = occ + rand_seq(rng, 33) + oracle.reverse_complement("iupac", occ)
        reads.append(tx)
    for k in (0, 2):
        want = ref.expected(lambda p, t: oracle.search("iupac", p, t, k, rc=True), pats, reads)
        by_pat = {}
        for w in want:
            by_pat.setdefault((w[1], w[7]), []).append(w)
        assert len(by_pat.get((2, "+"), [])) >= 10 and (5, "+") not in by_pat and (5, "-") not in by_pat
        assert len(by_pat.get((6, "+"), [])) >= 10 and (6, "-") not in by_pat and len(by_pat.get((1, "-"), [])) >= 5
        # the rule bites: a read with the barcode twice reports the later forward occurrence / the earlier Rc one
        assert sum(1 for w in want if w[7] == "+" and w[2] > 60) >= 10 and sum(1 for w in want if w[7] == "-" and w[2] < 40) >= 10
        for seeded in (1, 0):
            s = sassy.Searcher("iupac", rc=True)
            s.set_option("many_tiled", 1)
            s.set_option("many_seeded", seeded)
            check(s, pats, reads, k, want, ("ties", k, seeded), device_stats=(5, 6))


def test_low_complexity_reads(sassy):
    """Poly-A, microsatellites, N runs: long plateaus of equal cost, minima at the very end of a text and in front of the
    next one's start."""
    rng = random.Random(9)
    units = [b"A", b"AC", b"AAT", b"CAG", b"ACGT", b"GATA"]
    m = 18
    pats = [(u * m)[:m] for u in units] + [rand_seq(rng, m) for _ in range(4)]
    pats.append(pats[1][:9] + b"N" + pats[1][10:])
    reads = []
    for i in range(240):
        u = units[i % len(units)]
        n = rng.choice([m - 3, m, m + 1, 40, 200])
        body = (u * n)[:n]
        kind = (i // 6) % 5
        if kind == 0:
            tx = body
        elif kind == 1:
            tx = rand_seq(rng, 5) + body
        elif kind == 2:
            tx = body + rand_seq(rng, 3)
        elif kind == 3:
            tx = body[:n // 2] + b"N" * rng.randrange(1, 25) + body[n // 2:]
        else:
            tx = body[:n // 2] + rand_seq(rng, 2) + body[n // 2:]
        reads.append(tx)
    for k in (0, 2, 6):
        for rc in (True, False):
            want = ref.expected(lambda p, t: oracle.search("iupac", p, t, k, rc=rc), pats, reads)
            assert len(want) >= 150
            for seeded in (1, 0):
                s = sassy.Searcher("iupac", rc=rc)
                s.set_option("many_tiled", 1)
                s.set_option("many_seeded", seeded)
                check(s, pats, reads, k, want, ("low complexity", k, rc, seeded), device_stats=(5, 6))


def test_text_batch_input(sassy):
    rng = random.Random(10)
    pats = [rand_seq(rng, 24) for _ in range(16)]
    reads = barcode_reads(rng, pats, 600, 2, 80, 400)
    reads[11] = b""
    want = ref.expected_fast("iupac", pats, reads, 2, True)
    s = sassy.Searcher("iupac", rc=True)
    check(s, pats, sassy.TextBatch.from_list(reads), 2, want, "text batch", host_texts=reads)


def test_general_path_shapes(sassy):
    """What goes to the general path whatever the switch says: Ascii forward, max_n_frac with N-rich reads, patterns of two
    lengths, a single text, device-resident texts."""
    rng = random.Random(11)
    # Ascii, forward
    letters = b"abcdefgh "
    apats = [rand_seq(rng, 12, letters) for _ in range(5)]
    atexts = []
    for i in range(60):
        tx = bytearray(rand_seq(rng, rng.randrange(0, 200), letters))
        if len(tx) > 60:
            ins = mutate(rng, apats[i % 5], i % 3, letters)
            tx[20:20 + len(ins)] = ins
            if i % 2:
                tx[45:45 + len(ins)] = ins
        atexts.append(bytes(tx))
    want = ref.expected(lambda p, t: oracle.search("ascii", p, t, 2), apats, atexts)
    assert len(want) >= 25
    check(sassy.Searcher("ascii", rc=False), apats, atexts, 2, want, "ascii")
    # max_n_frac = 0.2, reads with runs of N (the filter bites) and plain reads
    pats = [rand_seq(rng, 24) for _ in range(8)]
    nreads = []
    for i in range(150):
        tx = bytearray(rand_seq(rng, rng.randrange(60, 300)))
        ins = mutate(rng, pats[i % 8], i % 3)
        if i % 2:
            ins = oracle.reverse_complement("iupac", ins)
        at = rng.randrange(0, len(tx) - 30)
        tx[at:at + len(ins)] = ins
        if i % 3 == 0:
            a = rng.randrange(0, len(tx) - 20)
            tx[a:a + rng.randrange(6, 20)] = b"N" * rng.randrange(6, 20)
        nreads.append(bytes(tx))
    want = ref.expected(lambda p, t: oracle.search_modes("iupac", p, t, 3, rc=True, max_n_frac=0.2), pats, nreads)
    free = ref.expected(lambda p, t: oracle.search("iupac", p, t, 3, rc=True), pats, nreads)
    assert len(want) >= 100 and want != free
    # (without trace the N filter sees the end position only: other records survive -- the traced comparison is the case)
    s = sassy.Searcher("iupac", rc=True).with_max_n_frac(0.2)
    for dev in (1, 0):
        s.set_option("best_match_device", dev)
        assert [ref.got_record(m) for m in s.best_matches(pats, nreads, 3)] == want, ("max_n_frac", dev)
    # patterns of two lengths
    pats2 = pats[:4] + [rand_seq(rng, 16) for _ in range(3)]
    reads2 = [r if i % 2 else r[:40] + pats2[4 + i % 3] + r[40:] for i, r in enumerate(nreads[1:60:2])]
    want = ref.expected(lambda p, t: oracle.search("iupac", p, t, 2, rc=True), pats2, reads2)
    assert {len(pats2[w[1]]) for w in want} == {16, 24}
    check(sassy.Searcher("iupac", rc=True), pats2, reads2, 2, want, "two lengths")
    # a single text
    want = ref.expected(lambda p, t: oracle.search("iupac", p, t, 3, rc=True), pats, nreads[1:2])
    assert len(want) == 1
    check(sassy.Searcher("iupac", rc=True), pats, nreads[1:2], 3, want, "one text")

    # device-resident texts
    class _DevText:
        """Minimal stand-in for a device tensor: data_ptr / numel / is_cuda."""

        def __init__(self, ptr, n):
            self._p, self._n, self.is_cuda = ptr, n, True
            self.dtype = type("_DT", (), {"itemsize": 1})()

        def data_ptr(self):
            return self._p

        def numel(self):
            return self._n

        def is_contiguous(self):
            return True

    host = [nreads[1], b"", nreads[4], nreads[2] + nreads[5]]   # (plain reads; barcodes on either strand)
    offs, total = [], 0
    for t in host:
        offs.append(total)
        total += (len(t) + 15) // 16 * 16 + 64
    buf = sassy.DeviceBuffer(total + 256)
    try:
        for t, off in zip(host, offs):
            if t:
                buf.upload(t, off)
        dev = [_DevText(buf.ptr + off, len(t)) for t, off in zip(host, offs)]
        for profile, rc in (("dna", False), ("iupac", True)):
            want = ref.expected(lambda p, t: oracle.search(profile, p, t, 3, rc=rc), pats, host)
            assert len(want) >= 2
            check(sassy.Searcher(profile, rc=rc), pats, dev, 3, want, ("device texts", profile, rc), host_texts=host)
    finally:
        buf.free()


def test_invalid_arguments(sassy):
    import ctypes as C
    pats, texts = [b"ACGTACGTAC", b"TTGACCATGA"], [b"ACGTACGTACGT", b"GGGG"]
    s = sassy.Searcher("iupac", rc=True)
    with pytest.raises(sassy.SassyHipError, match="k must be <= 254"):
        s.best_matches(pats, texts, 255)
    with pytest.raises(sassy.SassyHipError, match="reverse complement is not defined"):
        sassy.Searcher("ascii", rc=True).best_matches(pats, texts, 1)
    pp, pl, n_patterns, tp, tl, n_texts, _, _alive = s._marshal_many(pats, texts)
    out = C.c_void_p()
    for flags in (sassy.ALL_MINIMA, 8, 1 << 20):
        assert sassy.lib().sassy_hip_best_matches(s._h, pp, pl, n_patterns, tp, tl, n_texts, 1, flags, C.byref(out)) == -1, flags
        with pytest.raises(sassy.SassyHipError, match="SASSY_HIP_TEXT_ON_DEVICE and SASSY_HIP_WITHOUT_TRACE only"):
            sassy._check(-1)
    assert len(s.best_matches(pats, texts, 1)) == 1  # (and the searcher still works)


def test_cli_search_best(sassy, tmp_path):
    """`search --best` on a small FASTQ: exactly the rows the definition selects from the rows of plain `search`."""
    rng = random.Random(12)
    pats = [rand_seq(rng, 20) for _ in range(6)]
    pats[4] = pats[1]
    (tmp_path / "p.txt").write_bytes(b"".join(p + b"\n" for p in pats))
    recs = []
    for i in range(90):
        tx = bytearray(rand_seq(rng, rng.randrange(80, 300)))
        if i % 4 != 3:
            for j in range(1 + i % 3):
                ins = mutate(rng, pats[(i + j) % 6], (i + j) % 3)
                if (i + j) % 2:
                    ins = oracle.reverse_complement("iupac", ins)
                at = rng.randrange(0, len(tx) - 25)
                tx[at:at + len(ins)] = ins
        recs.append((b"read%d" % i, bytes(tx)))
    (tmp_path / "r.fq").write_bytes(b"".join(b"@" + i + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in recs))
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(*argv):
        p = subprocess.run([sys.executable, "-m", "sassy_amd", "search", "-l", str(tmp_path / "p.txt"), "-k", "2"] + list(argv) +
                           [str(tmp_path / "r.fq")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        return p.stdout.splitlines()

    for extra in ([], ["--max-n-frac", "1.0"], ["--no-rc", "-a", "dna"]):
        rows, best = run(*extra), run("--best", *extra)
        assert rows[0] == best[0] and rows[0].startswith("pat_id\ttext_id")
        by_text = {}
        for row in rows[1:]:
            pat_id, text_id, cost, strand, start, end = row.split("\t")[:6]
            rc = strand == "-"
            key = (int(cost), int(pat_id), rc, int(start) if rc else -int(end))
            if text_id not in by_text or key < by_text[text_id][0]:
                by_text[text_id] = (key, row)
        order = [i.decode() for i, _ in recs]
        want = [by_text[t][1] for t in order if t in by_text]
        assert len(want) >= 40 and len(want) < len(rows) - 1
        assert best[1:] == want, (extra, best[1:4], want[:3])
