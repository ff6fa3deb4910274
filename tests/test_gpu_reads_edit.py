"""The edit-distance batch calls over a resident read batch (sassy_hip_search_many_reads, _min_costs_reads, _best_pattern_reads,
_best_matches_reads; sassy_amd/csrc/reads_relayout.hip) on the GPU.

The relayout kernel's buffer is compared byte for byte with the numpy layout (tests/helpers/relayout_ref.py); each of the four
calls on DeviceReads(raw) must equal its sibling on the host list of the same sequences, record by record and cigar by cigar
and in the same order, and both must equal the CPU oracle (tests/helpers/best_matches_ref.py for the best record per read).
A resident call that took the pair loop instead of a one-pass path shows in stats(): `filtered` and `scan_launches` must be the
host-list call's.

relayout_ref.LENGTHS alone never puts a start of the separator layout on residue 15 mod 16 or 63 mod 64 (its lengths in
front of any read sum to 0, 1 or 2 mod 16 in either order); relayout_ref.MORE_LENGTHS adds those; every case of the first list stays.
The refusal "a handle made on another device" needs two devices to be provoked; on a box with one it cannot be made to
happen and that single line is not exercised there."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import best_matches_ref as bref  # noqa: E402
import relayout_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    assert sassy_amd.device_count() > 0, "no HIP device: the GPU tests must not silently skip"
    return sassy_amd


def fastq_of(seqs, eol=b"\n"):
    return b"".join(b"@r%d x" % i + eol + s + eol + b"+" + eol + bytes(33 + (i + j) % 40 for j in range(len(s))) + eol for i, s in enumerate(seqs))


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


# ---------------------------------------------------------------- 1. the buffer, byte for byte
def test_relayout_buffer_byte_for_byte(sassy):
    L = sassy.lib()
    mod16, mod64, cases = set(), set(), 0
    for order, lens in (("forward", ref.LENGTHS), ("reversed", ref.LENGTHS[::-1]), ("more", ref.MORE_LENGTHS)):
        seqs = ref.sequences(lens)
        reads = sassy.DeviceReads(fastq_of(seqs))
        before = reads.download_text()
        assert reads.seq_lens.tolist() == lens
        for first, count in ((0, len(lens)), (3, 5)):
            part = seqs[first:first + count]
            for name, starts, total, pad in ref.geometries([len(s) for s in part]):
                mod16 |= set((starts % 16).tolist())
                mod64 |= set((starts % 64).tolist())
                want = ref.layout(part, starts, total, pad)
                buf = sassy.DeviceBuffer(total + 64)
                buf.upload(b"\xEE" * (total + 64))
                st = np.ascontiguousarray(starts, dtype=np.uint64)
                rc = L.sassy_hip_reads_relayout(reads._handle(), first, count, st.ctypes.data, total, pad, buf.ptr, None)
                assert rc == 0, (order, name, first, L.sassy_hip_last_error())
                got = np.frombuffer(buf.download(total + 64), dtype=np.uint8)
                buf.free()
                msg = ref.first_difference(got[:total], want, starts, first)
                assert msg is None, (order, name, first, count, msg)
                assert (got[total:] == 0xEE).all(), (order, name, first, "bytes behind total were written")
                cases += 1
        assert reads.download_text() == before
        reads.free()
    assert cases == 24 and {0, 1, 15} <= mod16 and {0, 63} <= mod64, (cases, sorted(mod16), sorted(mod64))


def test_relayout_refusals(sassy):
    L = sassy.lib()
    reads = sassy.DeviceReads(fastq_of([b"ACGT", b"", b"GGGTTT"]))
    buf = sassy.DeviceBuffer(4096)
    ok = np.array([0, 64, 64], dtype=np.uint64)

    def call(h=None, first=0, count=3, starts=ok, total=128, ptr=None):
        return L.sassy_hip_reads_relayout(reads._handle() if h is None else h, first, count, None if starts is None else starts.ctypes.data,
                                          total, ord("X"), buf.ptr if ptr is None else ptr, None)
    assert call() == 0
    assert buf.download(128) == b"ACGT" + b"X" * 60 + b"GGGTTT" + b"X" * 58
    for bad in (dict(h=C.c_void_p(None)), dict(starts=None), dict(ptr=C.c_void_p(None)), dict(first=1, count=3), dict(first=4, count=0),
                dict(ptr=buf.ptr + 8), dict(starts=np.array([0, 2, 64], dtype=np.uint64)), dict(total=66),
                dict(starts=np.array([64, 0, 64], dtype=np.uint64))):
        assert call(**bad) == -1, bad
    buf.free()
    reads.free()


# ---------------------------------------------------------------- the comparison of the four calls
def mkey(m):
    return (m.pattern_idx, m.text_idx, m.text_start, m.text_end, m.pattern_start, m.pattern_end, m.cost, m.strand, m.cigar)


class Oracle:
    """The oracle's matches of every (pattern, read) pair, computed once per read set and left unchanged."""

    def __init__(self, profile, pats, seqs, k, rc, alpha=None):
        def search(p, t, allm):
            if alpha is None:
                return oracle.search(profile, p, t, k, rc=rc, all_minima=allm)
            return oracle.search_overhang(profile, p, t, k, alpha, rc=rc, all_minima=allm)
        self.pats, self.seqs, self.m = pats, seqs, len(pats[0])
        self.plain = {(pi, ti): search(p, t, False) for pi, p in enumerate(pats) for ti, t in enumerate(seqs)}
        self.all = {(pi, ti): search(p, t, True) for pi, p in enumerate(pats) for ti, t in enumerate(seqs)}

    def records(self, table):
        return sorted((pi, ti, m.text_start, m.text_end, m.pattern_start, m.pattern_end, m.cost, m.strand, m.cigar)
                      for (pi, ti), ms in table.items() for m in ms)

    def untraced(self):
        return sorted((pi, ti, m.text_start if m.strand == "-" else NONE, NONE if m.strand == "-" else m.text_end, NONE, m.pattern_end, m.cost,
                       m.strand, "") for (pi, ti), ms in self.plain.items() for m in ms)

    def min_costs(self):
        cost = np.full((len(self.pats), len(self.seqs)), 255, np.uint8)
        strand = np.zeros((len(self.pats), len(self.seqs)), np.uint8)
        for (pi, ti), ms in self.plain.items():
            if ms:
                c, sd = min((m.cost, 1 if m.strand == "-" else 0) for m in ms)
                cost[pi, ti], strand[pi, ti] = c, sd
        return cost, strand

    def best(self):
        return bref.expected(lambda p, t: self.plain[(self.pats.index(p), self.seqs.index(t))], self.pats, self.seqs)


def four_calls(sassy, make, pats, seqs, raw, k, orc, ctx, filtered=None):
    """Every call on DeviceReads(raw), on the host list and from the oracle.  make(): a fresh searcher with the options set."""
    reads = sassy.DeviceReads(raw)
    assert [reads.download(i) for i in (0, len(seqs) // 2, len(seqs) - 1)] == [seqs[0], seqs[len(seqs) // 2], seqs[-1]]
    text_before = reads.download_text()
    s_host, s_dev = make(), make()
    pats_u = list(dict.fromkeys(pats))
    assert pats_u == pats, "the oracle's table is keyed by pattern"

    def both(call):
        host = call(s_host, seqs)
        st_host = s_host.stats()
        dev = call(s_dev, reads)
        st_dev = s_dev.stats()
        assert st_dev["scan_launches"] == st_host["scan_launches"] and st_dev["filtered"] == st_host["filtered"], \
            (ctx, "the resident call took another path", st_dev["filtered"], st_host["filtered"], st_dev["scan_launches"], st_host["scan_launches"])
        if filtered is not None:
            assert st_dev["filtered"] == filtered, (ctx, st_dev["filtered"], filtered)
        return host, dev

    for name, kw, want in (("search_many", {}, orc.records(orc.plain)), ("search_all", dict(all_minima=True), orc.records(orc.all)),
                           ("without trace", dict(without_trace=True), orc.untraced())):
        host, dev = both(lambda s, t: [mkey(m) for m in s.search_many(pats, t, k, **kw)])
        print(ctx, name, "records", len(dev), "host", len(host), "oracle", len(want))
        assert dev == host, (ctx, name, len(dev), len(host), [(a, b) for a, b in zip(dev, host) if a != b][:2])
        assert sorted(host) == want, (ctx, name, len(host), len(want), sorted(set(host) ^ set(want))[:4])
        assert len(want) > 0, (ctx, name)
    (hc, hs), (dc, ds) = both(lambda s, t: s.min_costs(pats, t, k, strands=True))
    wc, ws = orc.min_costs()
    assert np.array_equal(dc, hc) and np.array_equal(ds, hs) and np.array_equal(hc, wc) and np.array_equal(hs, ws), (ctx, "min_costs")
    best = orc.best()
    host, dev = both(lambda s, t: tuple(a.tolist() for a in s.best_pattern(pats, t, k)))
    wcost, wpat, wstrand = [255] * len(seqs), [0xFFFFFFFF] * len(seqs), [0] * len(seqs)
    for w in best:
        wcost[w[0]], wpat[w[0]], wstrand[w[0]] = w[6], w[1], 1 if w[7] == "-" else 0
    assert dev == host == (wcost, wpat, wstrand), (ctx, "best_pattern")
    host, dev = both(lambda s, t: [bref.got_record(m) for m in s.best_matches(pats, t, k)])
    assert dev == host == best, (ctx, "best_matches", len(dev), len(host), len(best))
    host, dev = both(lambda s, t: [bref.got_record(m) for m in s.best_matches(pats, t, k, without_trace=True)])
    assert dev == host == [bref.without_trace(w) for w in best], (ctx, "best_matches without trace")
    assert reads.download_text() == text_before, (ctx, "the handle was written")
    reads.free()
    return best


def plant(rng, pats, n_reads, k, m):
    """Reads of 0 .. 200 bytes with a variant of a pattern -- a substitution, an insertion or a deletion, or none -- at the
    read's start, in its middle and at its very end, on either strand; reads shorter than m, of exactly m, and empty ones."""
    seqs = []
    for i in range(n_reads):
        n = [0, 1, m - 1, m, m + 1, 23, 64, 65, 200][i % 9] if i % 4 == 0 else rng.randrange(m + 4, 201)
        tx = bytearray(rand_seq(rng, n))
        occ = bytearray(pats[i % len(pats)])
        kind, at = (i // 3) % 4, rng.randrange(2, m - 2)
        if kind == 0:
            occ[at] = (set(b"ACGT") - {occ[at]}).pop()
        elif kind == 1:
            occ.insert(at, rng.choice(b"ACGT"))
        elif kind == 2:
            del occ[at]
        if (i // 2) % 2:
            occ = bytearray(oracle.reverse_complement("iupac", bytes(occ)))
        if n >= len(occ) and i % 7 != 6:
            where = i % 3
            pos = 0 if where == 0 else n - len(occ) if where == 1 else rng.randrange(0, n - len(occ) + 1)
            tx[pos:pos + len(occ)] = occ
        seqs.append(bytes(tx))
    return seqs


@pytest.fixture(scope="module")
def barcodes():
    rng = random.Random(20261020)
    pats = [rand_seq(rng, 24) for _ in range(8)]
    seqs = plant(rng, pats, 300, 3, 24)
    assert {0, 23, 24} <= {len(s) for s in seqs} and max(len(s) for s in seqs) <= 200
    return pats, seqs, fastq_of(seqs), Oracle("iupac", pats, seqs, 3, True)


# ---------------------------------------------------------------- 2. the four calls, both one-pass scans
@pytest.mark.parametrize("mode", ("seeded", "tiled"))
def test_four_calls_equal_siblings_and_oracle(sassy, barcodes, mode):
    pats, seqs, raw, orc = barcodes

    def make():
        s = sassy.Searcher("iupac", rc=True)
        if mode == "seeded":
            s.set_option("many_seeded", 1)
        else:
            s.set_option("many_seeded", 0).set_option("many_tiled", 1)
        return s
    best = four_calls(sassy, make, pats, seqs, raw, 3, orc, mode, filtered=6 if mode == "seeded" else 5)
    assert len(best) >= 150 and sum(1 for w in best if w[7] == "-") >= 40
    # variants at the very start and the very end of a read were found
    assert any(w[2] == 0 for w in best) and any(w[3] == len(seqs[w[0]]) for w in best)


# ---------------------------------------------------------------- 3. one pattern: a chain per strand
@pytest.mark.parametrize("rc", (False, True))
def test_one_pattern_chains(sassy, rc):
    rng = random.Random(3)
    pats = [rand_seq(rng, 32)]
    seqs = plant(rng, pats, 120, 3, 32)
    orc = Oracle("iupac", pats, seqs, 3, rc)
    four_calls(sassy, lambda: sassy.Searcher("iupac", rc=rc), pats, seqs, fastq_of(seqs), 3, orc, ("one pattern", rc))


# ---------------------------------------------------------------- 4. overhang
@pytest.mark.parametrize("seeded", (1, 0))
def test_overhang_at_block_borders(sassy, seeded):
    """alpha = 0.5: the per-text layout gives a read roundup64(len + steps) bytes, steps = 24 + 2 virtual columns; reads of
    63, 64, 65 and 64 - steps - 1, 64 - steps, 64 - steps + 1 bytes sit around the slot sizes' borders."""
    rng = random.Random(4)
    alpha, k, m, steps = 0.5, 3, 24, 26
    pats = [rand_seq(rng, m) for _ in range(6)]
    seqs = []
    for i, n in enumerate([63, 64, 65, 64 - steps - 1, 64 - steps, 64 - steps + 1] * 6):
        tx = bytearray(rand_seq(rng, n))
        occ, cut = pats[i % 6], 2 + i % 5
        if (i // 6) % 2:
            occ = oracle.reverse_complement("iupac", occ)
        if (i // 12) % 3 == 0:
            tx[0:m - cut] = occ[cut:]            # hangs over the read's start
        elif (i // 12) % 3 == 1:
            tx[n - (m - cut):] = occ[:m - cut]   # ... over its end
        seqs.append(bytes(tx))
    orc = Oracle("iupac", pats, seqs, k, True, alpha=alpha)

    def make():
        return sassy.Searcher("iupac", rc=True, alpha=alpha).set_option("overhang_seeded", seeded)
    best = four_calls(sassy, make, pats, seqs, fastq_of(seqs), k, orc, ("overhang", seeded), filtered=6 if seeded else 5)
    assert sum(1 for w in best if w[5] < m) >= 6 and sum(1 for w in best if w[4] > 0) >= 6  # over the end / over the start


# ---------------------------------------------------------------- 5. other profiles
def same_as_host_list(sassy, make, pats, seqs, raw, k, ctx):
    reads = sassy.DeviceReads(raw)
    s_host, s_dev = make(), make()
    out = []
    for call in (lambda s, t: [mkey(m) for m in s.search_many(pats, t, k)],
                 lambda s, t: [a.tolist() for a in s.min_costs(pats, t, k, strands=True)],
                 lambda s, t: [a.tolist() for a in s.best_pattern(pats, t, k)],
                 lambda s, t: [bref.got_record(m) for m in s.best_matches(pats, t, k)]):
        host, dev = call(s_host, seqs), call(s_dev, reads)
        assert dev == host, (ctx, len(dev), len(host))
        out.append(host)
    reads.free()
    return out


def test_dna_batch_with_an_n_and_ascii_prose(sassy):
    rng = random.Random(5)
    pats = [rand_seq(rng, 24) for _ in range(8)]
    seqs = plant(rng, pats, 60, 3, 24)
    want = [(pi, ti) + (m.text_start, m.text_end, m.pattern_start, m.pattern_end, m.cost, m.strand, m.cigar)
            for pi, p in enumerate(pats) for ti, t in enumerate(seqs) for m in oracle.search("dna", p, t, 3, rc=True)]
    # plain: a one-pass path; with one N in one read the Dna searcher declines it -- for the resident batch as for the host list
    # (a zero byte INSIDE a sequence counts as another letter, as for the host list; the zeros between the reads do not)
    paths = {}
    for odd in (None, b"N", b"\0"):
        ss = list(seqs)
        if odd:
            assert len(ss[17]) > 6
            ss[17] = ss[17][:5] + odd + ss[17][6:]
        got = same_as_host_list(sassy, lambda: sassy.Searcher("dna", rc=True), pats, ss, fastq_of(ss), 3, ("dna", odd))
        if not odd:
            assert sorted(got[0]) == sorted(want) and len(want) >= 30
        for name, texts in (("host", ss), ("resident", sassy.DeviceReads(fastq_of(ss)))):
            s = sassy.Searcher("dna", rc=True).set_option("many_tiled", 1)
            s.search_many(pats, texts, 3)
            paths[(odd, name)] = s.stats()["filtered"]
    # the decision made on the device is the host's: the one-pass scan for plain reads, not with another letter
    assert paths[(None, "host")] in (5, 6) and all(paths[(o, "resident")] == paths[(o, "host")] for o in (None, b"N", b"\0")), paths
    assert paths[(b"N", "host")] not in (5, 6) and paths[(b"\0", "host")] not in (5, 6), paths
    words = b"the quick brown fox jumps over the lazy dog and runs off into the forest where nobody has ever seen it again".split()
    apats = [b"quick brown fox", b"the lazy dog and", b"into the forest "]
    prose = []
    for i in range(50):
        line = [rng.choice(words) for _ in range(rng.randrange(0, 30))]
        if i % 2 == 0:  # a phrase with a typo, among the words
            phrase = bytearray(apats[i % 3])
            phrase[rng.randrange(len(phrase))] = ord("z")
            line.insert(rng.randrange(len(line) + 1), bytes(phrase))
        prose.append(b" ".join(line))
    got = same_as_host_list(sassy, lambda: sassy.Searcher("ascii", rc=False), apats, prose, fastq_of(prose), 2, "ascii")
    want = [(pi, ti) + (m.text_start, m.text_end, m.pattern_start, m.pattern_end, m.cost, m.strand, m.cigar)
            for pi, p in enumerate(apats) for ti, t in enumerate(prose) for m in oracle.search("ascii", p, t, 2)]
    assert sorted(got[0]) == sorted(want) and len(want) >= 10


# ---------------------------------------------------------------- 6. several batches
def test_several_batches(sassy):
    rng = random.Random(6)
    pats = [rand_seq(rng, 24) for _ in range(8)]
    seqs = [(s + rand_seq(rng, 330))[:270 + (7 * i) % 60] for i, s in enumerate(plant(rng, pats, 40, 3, 24))]
    assert 250 <= sum(len(s) for s in seqs) // len(seqs) <= 350

    def make():
        return sassy.Searcher("iupac", rc=True).set_option("many_batch", 4096).set_option("many_tiled", 1)
    got = same_as_host_list(sassy, make, pats, seqs, fastq_of(seqs), 3, "several batches")
    one = sassy.Searcher("iupac", rc=True).set_option("many_tiled", 1)
    assert got[0] == [mkey(m) for m in one.search_many(pats, seqs, 3)] and len(got[0]) >= 20
    assert got[3] == [bref.got_record(m) for m in one.best_matches(pats, seqs, 3)]
    # more than one batch was scanned: two launches (one per strand) per batch of at most 4096 bytes
    s = make()
    reads = sassy.DeviceReads(fastq_of(seqs))
    s.search_many(pats, reads, 3)
    assert s.stats()["scan_launches"] >= 2 * 3, s.stats()["scan_launches"]
    reads.free()


# ---------------------------------------------------------------- 7. one handle, many calls
def test_one_handle_many_calls(sassy, barcodes):
    pats, seqs, raw, _ = barcodes
    rng = random.Random(7)
    others = [rand_seq(rng, 20) for _ in range(5)] + [seqs[50][10:30]]
    exact = [p[:16] for p in pats]
    reads = sassy.DeviceReads(raw)
    before = reads.download_text()
    s = sassy.Searcher("iupac", rc=True)
    got = ([a.tolist() for a in s.best_pattern(pats, reads, 3)], [mkey(m) for m in s.search_many(others, reads, 2)],
           [a.tolist() for a in s.hamming_best_pattern(exact, reads, 1)])
    assert reads.download_text() == before
    for i, call in enumerate((lambda s, t: [a.tolist() for a in s.best_pattern(pats, t, 3)],
                              lambda s, t: [mkey(m) for m in s.search_many(others, t, 2)],
                              lambda s, t: [a.tolist() for a in s.hamming_best_pattern(exact, t, 1)])):
        fresh = sassy.DeviceReads(raw)
        assert call(sassy.Searcher("iupac", rc=True), fresh) == got[i], i
        fresh.free()
        assert call(sassy.Searcher("iupac", rc=True), seqs) == got[i], i
    assert len(got[1]) >= 1
    reads.free()


# ---------------------------------------------------------------- 8. refusals
def test_refusals(sassy):
    L = sassy.lib()
    reads = sassy.DeviceReads(fastq_of([b"ACGTACGTACGTACGTACGT", b"ACGTTTTTACGTACGTAAAA"]))
    s = sassy.Searcher("iupac", rc=True)
    pp, pl = (C.c_char_p * 1)(b"ACGTACGT"), (C.c_size_t * 1)(8)
    out, cost = C.c_void_p(), (C.c_uint8 * 8)()
    calls = (("search_many_reads", (C.byref(out),)), ("min_costs_reads", (cost, None)), ("best_pattern_reads", (cost, None, None)),
             ("best_matches_reads", (C.byref(out),)))

    def run(name, tail, searcher, handle, flags=0):
        return getattr(L, "sassy_hip_" + name)(searcher._h, pp, pl, 1, handle, 1, flags, *tail)
    for name, tail in calls:
        assert run(name, tail, s, None) == -1 and b"null" in L.sassy_hip_last_error().lower(), name
        assert run(name, tail, s, reads._handle(), sassy.TEXT_ON_DEVICE) == -1 and b"TEXT_ON_DEVICE" in L.sassy_hip_last_error(), name
    # the sibling's own refusals, with its codes: an unknown flag, k > 254, LINE_SPANS
    assert run("min_costs_reads", calls[1][1], s, reads._handle(), sassy.ALL_MINIMA) == -1
    assert run("best_matches_reads", calls[3][1], s, reads._handle(), sassy.ALL_MINIMA) == -1
    assert L.sassy_hip_best_pattern_reads(s._h, pp, pl, 1, reads._handle(), 255, 0, cost, None, None) == -1
    assert run("search_many_reads", calls[0][1], s, reads._handle(), sassy.LINE_SPANS) == -3
    a = sassy.Searcher("ascii", rc=True)
    assert run("search_many_reads", calls[0][1], a, reads._handle()) == -3 and b"reverse complement" in L.sassy_hip_last_error()
    # open tickets
    text = rand_seq(random.Random(8), 4096)
    buf = sassy.DeviceBuffer(len(text) + 64)
    buf.upload(text)
    t = sassy.Searcher("dna", rc=False)
    ticket = t.search_shard_begin(text[100:120], buf.ptr, 0, len(text), 0, len(text), 1)
    for name, tail in calls:
        assert run(name, tail, t, reads._handle()) == -1 and b"in flight" in L.sassy_hip_last_error(), name
    assert len(t.search_finish(ticket).matches) >= 1
    buf.free()
    # a handle made on another device than the searcher's
    if sassy.device_count() >= 2:
        far = sassy.Searcher("iupac", rc=True)
        far.set_device(1)
        for name, tail in calls:
            assert run(name, tail, far, reads._handle()) == -1 and b"made on device" in L.sassy_hip_last_error(), name
    else:
        with pytest.raises(sassy.SassyHipError, match="no such"):
            sassy.Searcher("iupac", rc=True).set_device(1)  # (one device: there is no other one to make the searcher on)
    # valid arguments still work afterwards, and an empty handle gives empty results
    assert len(s.search_many([b"ACGTACGT"], reads, 1)) >= 2
    empty = sassy.DeviceReads(b"")
    assert s.search_many([b"ACGTACGT"], empty, 1) == [] and s.best_matches([b"ACGTACGT"], empty, 1) == []
    assert s.min_costs([b"ACGTACGT"], empty, 1).shape == (1, 0) and s.best_pattern([b"ACGTACGT"], empty, 1)[0].size == 0
    empty.free()
    reads.free()
