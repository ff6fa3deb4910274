"""Best-cost search on the GPU (sassy_hip_min_costs / sassy_hip_best_pattern, `python -m sassy_amd filter`) against the
CPU oracle: want[p][t] = min(m.cost for m in oracle.search(alphabet, p, t, k, rc=...)), 255 if there is no match, the
strand of that minimum Fwd on a tie; best_pattern derived from want (lowest cost, lowest index, Fwd first).  Exact
equality, every case for both calls and for min_cost_device 1 (the device reduction of the scan's list where a one-pass
batch path takes the call) and 0 (search_many's records reduced by the host)."""
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = 255


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    assert sassy_amd.device_count() > 0, "no HIP device: the GPU tests must not silently skip"
    return sassy_amd


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, edits):
    s = bytearray(s)
    for _ in range(edits):
        t, p = rng.randrange(3), rng.randrange(len(s))
        if t == 0:
            s[p] = rng.choice(b"ACGT")
        elif t == 1:
            s.insert(p, rng.choice(b"ACGT"))
        elif len(s) > 1:
            del s[p]
    return bytes(s)


def pair_min(matches):
    """(cost, strand) of the cheapest match, Fwd on a tie; (255, 0) if there is none."""
    best = (NO, 0)
    for m in matches:
        best = min(best, (m.cost, 1 if m.strand in ("-", 1) else 0))
    return best


def want_matrix(search, pats, texts):
    """search(p, t) -> the oracle's matches of one pair."""
    cost = np.full((len(pats), len(texts)), NO, dtype=np.uint8)
    strand = np.zeros((len(pats), len(texts)), dtype=np.uint8)
    for pi, p in enumerate(pats):
        for ti, t in enumerate(texts):
            cost[pi, ti], strand[pi, ti] = pair_min(search(p, t))
    return cost, strand


def want_matrix_fast(profile, pats, texts, k, rc):
    """The same through the oracle's C entry point without a Python object per match (a read set: 10^5 pairs), texts
    shared out over threads (the oracle call releases the GIL)."""
    L = oracle.lib()
    prof = oracle._profile(profile)
    cost = np.full((len(pats), len(texts)), NO, dtype=np.uint8)
    strand = np.zeros((len(pats), len(texts)), dtype=np.uint8)

    def column(ti):
        t = texts[ti]
        for pi, p in enumerate(pats):
            res = L.orc_search(prof, int(rc), 0, p, len(p), t, len(t), k)
            try:
                assert not L.orc_result_failed(res)
                ms = L.orc_result_matches(res)
                cost[pi, ti], strand[pi, ti] = pair_min(ms[i] for i in range(L.orc_result_len(res)))
            finally:
                L.orc_result_free(res)

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(column, range(len(texts))))
    return cost, strand


def best_of(cost, strand):
    """Per text: (cost, pattern, strand) by the tie rule; pattern 0xFFFFFFFF where nothing matches."""
    n = cost.shape[1]
    bc, bp, bs = np.full(n, NO, np.uint8), np.full(n, 0xFFFFFFFF, np.uint32), np.zeros(n, np.uint8)
    for t in range(n):
        if cost.shape[0] == 0:
            continue
        keys = [(int(cost[p, t]), p, int(strand[p, t])) for p in range(cost.shape[0])]
        c, p, s = min(keys)
        if c != NO:
            bc[t], bp[t], bs[t] = c, p, s
    return bc, bp, bs


def check(s, pats, texts, k, want, ctx, device_stats=None, n_filter=False):
    """Both calls, both paths, exactly the oracle's values.  device_stats: the `filtered` codes the device run must show
    (5 tiled scan, 6 seeded search) -- the one-pass path took the call -- AND the reduction ran there: at timing level 2
    trace_ms is the reduction launches' time with min_cost_device = 1, and 0 with min_cost_device = 0, where search_many
    runs without trace (n_filter: the searcher has max_n_frac set, so the general path traces)."""
    wc, ws = want
    bc, bp, bs = best_of(wc, ws)
    if device_stats:
        s.set_timing(2)
    for dev in (1, 0):
        s.set_option("min_cost_device", dev)
        try:
            gc, gs = s.min_costs(pats, texts, k, strands=True)
            st = s.stats()
            print(ctx, "dev", dev, "min_costs: matches", int((wc != NO).sum()), "mismatches", int((gc != wc).sum()), int((gs != ws).sum()))
            assert gc.shape == wc.shape and gc.dtype == np.uint8
            assert np.array_equal(gc, wc), (ctx, dev, np.argwhere(gc != wc)[:5], gc[gc != wc][:5], wc[gc != wc][:5])
            assert np.array_equal(gs, ws), (ctx, dev, np.argwhere(gs != ws)[:5])
            assert np.array_equal(s.min_costs(pats, texts, k), wc), (ctx, dev)
            if device_stats:
                assert st["filtered"] in device_stats and st["candidates"] > 0, (ctx, dev, st)
                assert st["trace_ms"] > 0 if dev else (n_filter or st["trace_ms"] == 0), (ctx, dev, st)
            c, p, sd = s.best_pattern(pats, texts, k)
            if device_stats:
                st = s.stats()
                assert st["trace_ms"] > 0 if dev else (n_filter or st["trace_ms"] == 0), (ctx, dev, "best_pattern", st)
            print(ctx, "dev", dev, "best_pattern: mismatches", int((c != bc).sum()), int((p != bp).sum()), int((sd != bs).sum()))
            assert np.array_equal(c, bc), (ctx, dev, np.flatnonzero(c != bc)[:5])
            assert np.array_equal(p, bp), (ctx, dev, np.flatnonzero(p != bp)[:5], p[p != bp][:5], bp[p != bp][:5])
            assert np.array_equal(sd, bs), (ctx, dev, np.flatnonzero(sd != bs)[:5])
        finally:
            s.set_option("min_cost_device", 1)


def barcode_reads(rng, pats, n_reads, k, lo=700, hi=1100):
    """Reads with a planted barcode at 0 .. k edits (either strand, anywhere, the two ends included) and reads without."""
    reads = []
    for i in range(n_reads):
        n = rng.randrange(lo, hi)
        tx = bytearray(rand_seq(rng, n))
        if i % 5 != 4:
            ins = mutate(rng, rng.choice(pats), rng.randrange(0, k + 1))
            if rng.random() < 0.5:
                ins = oracle.reverse_complement("iupac", ins)
            at = rng.choice([0, n - len(ins), rng.randrange(0, n - len(ins) + 1)])
            tx[at:at + len(ins)] = ins
        reads.append(bytes(tx))
    return reads


@pytest.mark.parametrize("profile", ["iupac", "dna"])
@pytest.mark.parametrize("rc", [False, True])
def test_barcodes_over_reads(sassy, profile, rc):
    """96 x 24-mers over a few thousand ~1 kb reads, k in {0, 1, 3}; the seeded search and the tiled scan forced in turn."""
    rng = random.Random(1234 + (profile == "dna") + 2 * rc)
    pats = [rand_seq(rng, 24) for _ in range(96)]
    reads = barcode_reads(rng, pats, 2000, 3)
    for k in (0, 1, 3):
        want = want_matrix_fast(profile, pats, reads, k, rc)
        assert (want[0] != NO).sum() >= (150 if k == 0 else 350)
        for mode, code in (("seeded", 6), ("tiled", 5)):
            s = sassy.Searcher(profile, rc=rc)
            s.set_option("many_tiled", 1)
            s.set_option("many_seeded", 1 if mode == "seeded" else 0)
            check(s, pats, reads, k, want, (profile, rc, k, mode), device_stats=(code,))
    # a TextBatch (one buffer + offsets) gives what the list gives
    s = sassy.Searcher(profile, rc=rc)
    assert np.array_equal(s.min_costs(pats, sassy.TextBatch.from_list(reads), 3), want[0])


def test_ties_lowest_pattern_then_forward(sassy):
    """The same barcode twice in the list, a palindromic barcode (Fwd cost = Rc cost), two barcodes at equal cost in one
    read: the packed key's order is (cost, pattern index, strand)."""
    rng = random.Random(77)
    half = rand_seq(rng, 12)
    palin = half + oracle.reverse_complement("iupac", half)
    assert oracle.reverse_complement("iupac", palin) == palin
    pats = [rand_seq(rng, 24) for _ in range(8)]
    pats[5] = pats[2]          # a duplicate: the lower index wins
    pats[6] = palin
    reads = []
    for i in range(300):
        tx = bytearray(rand_seq(rng, rng.randrange(200, 500)))
        which = [pats[2], palin, pats[1], pats[7]][i % 4]
        ins = mutate(rng, which, i % 3)
        at = rng.randrange(0, len(tx) - 30)
        tx[at:at + len(ins)] = ins
        if i % 4 >= 2:         # a second barcode at the same number of edits, on the other strand
            ins2 = oracle.reverse_complement("iupac", mutate(rng, pats[0], i % 3))
            tx += rand_seq(rng, 40) + ins2
        reads.append(bytes(tx))
    for k in (0, 2):
        want = want_matrix(lambda p, t: oracle.search("iupac", p, t, k, rc=True), pats, reads)
        bc, bp, bs = best_of(*want)
        assert (bp == 2).sum() >= 20 and (bp == 5).sum() == 0 and ((bp == 6) & (bs == 0)).sum() >= 20
        for seeded in (1, 0):
            s = sassy.Searcher("iupac", rc=True)
            s.set_option("many_tiled", 1)
            s.set_option("many_seeded", seeded)
            check(s, pats, reads, k, want, ("ties", k, seeded), device_stats=(6 if seeded else 5,))


def test_text_edges_and_shapes_the_batch_paths_decline(sassy):
    """A match ending in the last column of one text and one starting in the first column of the next (separators), empty
    texts, texts shorter than the pattern, an ambiguity letter in a barcode; then what only the general path takes: a
    single text, patterns of several lengths, no patterns, no texts."""
    rng = random.Random(5)
    m, k = 20, 2
    pats = [rand_seq(rng, m) for _ in range(6)]
    pats[3] = pats[3][:4] + b"N" + pats[3][5:9] + b"R" + pats[3][10:]
    plain = [bytes(c if c in b"ACGT" else 65 for c in p) for p in pats]
    texts = []
    for i in range(160):
        n = rng.choice([0, 1, m - 1, m, m + 1, 60, 200])
        tx = bytearray(rand_seq(rng, n))
        if n >= m + 1:
            a, b = mutate(rng, plain[i % 6], i % 3)[:n], mutate(rng, plain[(i + 1) % 6], (i + 1) % 3)[:n]
            if i % 2:
                tx[n - len(a):] = a   # ends in the last column ...
            else:
                tx[:len(b)] = b       # ... and the next text starts with one
        texts.append(bytes(tx))
    for profile, pp in (("iupac", pats), ("dna", plain)):
        for rc in (False, True):
            want = want_matrix(lambda p, t: oracle.search(profile, p, t, k, rc=rc), pp, texts)
            assert (want[0] != NO).sum() >= 60
            for tiled, seeded in ((1, 0), (1, 1), (-1, -1)):
                s = sassy.Searcher(profile, rc=rc)
                s.set_option("many_tiled", tiled)
                s.set_option("many_seeded", seeded)
                check(s, pp, texts, k, want, ("edges", profile, rc, tiled, seeded))
    # the general path
    s = sassy.Searcher("iupac", rc=True)
    one = [texts[-1] + plain[0] + rand_seq(rng, 50)]
    check(s, pats, one, k, want_matrix(lambda p, t: oracle.search("iupac", p, t, k, rc=True), pats, one), "one text")
    mixed = [plain[0], plain[1][:12], plain[2] + plain[3][:7], b"ACG"]
    tx = [t for t in texts if len(t) >= 60][:40] + [b""]
    want = want_matrix(lambda p, t: oracle.search("iupac", p, t, k, rc=True), mixed, tx)
    check(s, mixed, tx, k, want, "mixed lengths")   # (ACG with k = 2 < 3 = m)
    assert s.min_costs([], tx, 1).shape == (0, len(tx)) and s.min_costs(pats, [], 1).shape == (len(pats), 0)
    c, p, sd = s.best_pattern([], tx, 1)
    assert (c == NO).all() and (p == 0xFFFFFFFF).all() and (sd == 0).all()


@pytest.mark.parametrize("max_overhang", [None, 2])
def test_overhang_searchers(sassy, max_overhang):
    """alpha = 0.5 with and without max_overhang: barcodes hanging over either end of a read; the cost includes the
    overhang price.  The one-pass overhang paths (seeded inside + per-text tiled edges, per-text tiled scan alone) and
    the chains."""
    rng = random.Random(11 + (max_overhang or 0))
    m, k, alpha = 24, 3, 0.5
    pats = [rand_seq(rng, m) for _ in range(12)]
    texts = []
    for i in range(240):
        n = rng.choice([0, 5, m, 80, 150, 300, 300])
        tx = bytearray(rand_seq(rng, n))
        p = mutate(rng, pats[i % 12], i % 2)
        cut = rng.randrange(1, 7)   # (alpha = 0.5: up to 3 = k for the overhang; capped at 2 columns: 1 + 1 per further column)
        if n >= 80 and i % 4 == 0:
            tx[:len(p) - cut] = p[cut:]            # hangs over the left end
        elif n >= 80 and i % 4 == 1:
            tx[n - (len(p) - cut):] = p[:len(p) - cut]   # ... the right end
        elif n >= 80 and i % 4 == 2:
            at = rng.randrange(0, n - len(p))
            tx[at:at + len(p)] = p
        texts.append(bytes(tx))
    for rc in (False, True):
        want = want_matrix(lambda p, t: oracle.search_overhang("iupac", p, t, k, alpha, rc=rc, max_overhang=max_overhang), pats, texts)
        assert (want[0] != NO).sum() >= 60
        if max_overhang is not None:   # the cap bites: the capped cost model prices planted reads differently
            free = want_matrix(lambda p, t: oracle.search_overhang("iupac", p, t, k, alpha, rc=rc), pats, texts)
            assert (free[0] != want[0]).sum() >= 20
        for tiled, seeded in ((1, 1), (1, 0), (0, 0)):
            s = sassy.Searcher("iupac", rc=rc, alpha=alpha).with_max_overhang(max_overhang)
            s.set_option("overhang_tiled", tiled)
            s.set_option("overhang_seeded", seeded)
            check(s, pats, texts, k, want, ("overhang", max_overhang, rc, tiled, seeded), device_stats=(5, 6) if tiled else None)


def test_n_filter(sassy):
    """max_n_frac = 0.2: only matches that pass the N filter count (the oracle's restatement of the reference's filter, as
    tests/test_gpu_parity.py::test_reporting_modes uses it) -- reads with runs of N (the general path) and plain reads
    (the device reduction: the filter cannot touch a batch without other letters); with only_best_match as well."""
    rng = random.Random(31)
    m, k, frac = 24, 3, 0.2
    pats = [rand_seq(rng, m) for _ in range(8)]
    plain, dirty = [], []
    for i in range(200):
        tx = bytearray(rand_seq(rng, rng.randrange(100, 400)))
        ins = bytearray(mutate(rng, pats[i % 8], i % 4))
        at = rng.randrange(0, len(tx) - 40)
        tx[at:at + len(ins)] = ins
        plain.append(bytes(tx))
        for _ in range(rng.randrange(0, 9)):
            ins[rng.randrange(len(ins))] = ord("N")
        tx[at:at + len(ins)] = ins
        if i % 3 == 0:
            a = rng.randrange(0, len(tx) - 30)
            tx[a:a + 30] = b"N" * 30
        dirty.append(bytes(tx))
    for rc in (False, True):
        for only_best in (False, True):
            for name, reads in (("plain", plain), ("n runs", dirty)):
                want = want_matrix(lambda p, t: oracle.search_modes("iupac", p, t, k, rc=rc, max_n_frac=frac, only_best=only_best), pats, reads)
                free = want_matrix(lambda p, t: oracle.search("iupac", p, t, k, rc=rc), pats, reads)
                if name == "n runs" and not only_best:
                    assert (want[0] != free[0]).sum() >= 10   # the filter bites
                s = sassy.Searcher("iupac", rc=rc).with_max_n_frac(frac)
                s.set_option("many_tiled", 1)
                if only_best:
                    s.only_best_match()
                check(s, pats, reads, k, want, ("n filter", rc, only_best, name), device_stats=(5, 6) if name == "plain" else None, n_filter=True)


def test_ascii_and_device_resident_texts(sassy):
    """Ascii (general path; rc refused as search_many refuses it); texts that live on the device."""
    rng = random.Random(3)
    pats = [bytes(rng.choice(b"abcdefgh ") for _ in range(12)) for _ in range(5)]
    texts = []
    for i in range(60):
        tx = bytearray(rng.choice(b"abcdefgh ") for _ in range(rng.randrange(0, 200)))
        if len(tx) > 40:
            ins = mutate(rng, pats[i % 5], i % 3)
            tx[20:20 + len(ins)] = ins
        texts.append(bytes(tx))
    want = want_matrix(lambda p, t: oracle.search("ascii", p, t, 2), pats, texts)
    assert (want[0] != NO).sum() >= 30
    check(sassy.Searcher("ascii", rc=False), pats, texts, 2, want, "ascii")
    for f in (sassy.Searcher("ascii", rc=True).min_costs, sassy.Searcher("ascii", rc=True).best_pattern):
        with pytest.raises(sassy.SassyHipError, match="reverse complement is not defined"):
            f(pats, texts, 2)
    # device-resident texts (SASSY_HIP_TEXT_ON_DEVICE)
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

    dpats = [rand_seq(rng, 24) for _ in range(4)]
    lens = [5000, 0, 300, 64, 20000]
    offs, total, host = [], 0, []
    for ln in lens:
        offs.append(total)
        total += (ln + 15) // 16 * 16 + 64
    buf = sassy.DeviceBuffer(total + 256)
    for ln, off in zip(lens, offs):
        t = bytearray(rand_seq(rng, ln))
        if ln >= 300:
            for j, p in enumerate(dpats[:3]):
                ins = mutate(rng, p, j)
                if j == 1:
                    ins = oracle.reverse_complement("dna", ins)
                at = rng.randrange(0, ln - 30)
                t[at:at + len(ins)] = ins
        host.append(bytes(t[:ln]))
        if ln:
            buf.upload(host[-1], off)
    dev = [_DevText(buf.ptr + off, ln) for ln, off in zip(lens, offs)]
    try:
        for profile, rc in (("dna", False), ("iupac", True)):
            want = want_matrix(lambda p, t: oracle.search(profile, p, t, 2, rc=rc), dpats, host)
            assert (want[0] != NO).sum() >= 6
            check(sassy.Searcher(profile, rc=rc), dpats, dev, 2, want, ("device texts", profile, rc))
    finally:
        buf.free()


def test_reduction_of_the_records_and_the_path_taken(sassy):
    """A second, weaker witness: the new calls equal the reduction of search_many's own records.  And the path is the one
    claimed: with timing level 2 the device reduction reports its launches' time and the entries it reduced."""
    rng = random.Random(9)
    pats = [rand_seq(rng, 24) for _ in range(96)]
    reads = barcode_reads(rng, pats, 1500, 3)
    s = sassy.Searcher("iupac", rc=True)
    s.set_timing(2)
    gc, gs = s.min_costs(pats, reads, 3, strands=True)
    st = s.stats()
    print("stats of the device reduction:", {x: st[x] for x in ("filtered", "candidates", "scan_ms", "trace_ms", "total_ms")})
    assert st["filtered"] in (5, 6) and st["trace_ms"] > 0 and st["candidates"] > 0, st
    arr = s.search_many(pats, reads, 3, as_result=True).array
    wc = np.full(gc.shape, NO, np.int64)
    key = np.full(gc.shape, 2 * NO, np.int64)
    np.minimum.at(key, (arr["pattern_idx"].astype(np.int64), arr["text_idx"].astype(np.int64)),
                  2 * arr["cost"].astype(np.int64) + arr["strand"].astype(np.int64))
    hit = key < 2 * NO
    wc[hit] = key[hit] >> 1
    assert hit.sum() >= 1000 and np.array_equal(gc, wc.astype(np.uint8)) and np.array_equal(gs[hit], (key[hit] & 1).astype(np.uint8))
    assert not gs[~hit].any()
    c, p, sd = s.best_pattern(pats, reads, 3)
    assert s.stats()["trace_ms"] > 0
    assert np.array_equal(c, gc.min(axis=0))
    s.set_option("min_cost_device", 0)
    assert np.array_equal(s.min_costs(pats, reads, 3), gc)
    assert s.stats()["filtered"] in (5, 6)  # (the general path is search_many itself: the same scan, then its records)


def test_fuzz_slice_against_the_oracle(sassy):
    """A few hundred random small cases, fixed seed, all three alphabets, both paths (in the manner of tests/test_gpu_fuzz.py)."""
    rng = random.Random(20240607)
    cases = 0
    for it in range(240):
        profile = ("dna", "iupac", "ascii")[it % 3]
        rc = profile != "ascii" and bool(it & 1)
        same_len = it % 4 != 3
        m, k = rng.randrange(6, 40), rng.randrange(0, 4)
        k = min(k, m // 3)
        letters = b"ACGT" if profile != "ascii" else b"abcd"
        pats = [rand_seq(rng, m if same_len else rng.randrange(5, 40), letters) for _ in range(rng.randrange(1, 9))]
        texts = []
        for _ in range(rng.randrange(1, 12)):
            tx = bytearray(rand_seq(rng, rng.choice([0, 3, m, 50, 150, 400]), letters))
            if len(tx) > 45 and rng.random() < 0.8:
                ins = mutate(rng, rng.choice(pats), rng.randrange(0, k + 1)) if profile == "ascii" else \
                    bytes(mutate(rng, rng.choice(pats), rng.randrange(0, k + 1)))
                if rc and rng.random() < 0.5:
                    ins = oracle.reverse_complement(profile, ins)
                at = rng.choice([0, len(tx) - len(ins), rng.randrange(0, len(tx) - len(ins) + 1)])
                tx[at:at + len(ins)] = ins
            if profile == "iupac" and rng.random() < 0.2 and len(tx) > 10:
                tx[rng.randrange(len(tx))] = ord("N")
            texts.append(bytes(tx))
        kk = k if all(len(p) > k for p in pats) else 0
        want = want_matrix(lambda p, t: oracle.search(profile, p, t, kk, rc=rc), pats, texts)
        s = sassy.Searcher(profile, rc=rc)
        s.set_option("many_tiled", (1, 1, -1)[it % 3] if profile != "ascii" else -1)
        s.set_option("many_seeded", (1, 0, -1)[(it // 3) % 3])
        check(s, pats, texts, kk, want, ("fuzz", it, profile, rc, m, kk))
        cases += 1
    assert cases == 240


def test_filter_cli_end_to_end(sassy, tmp_path):
    """`filter` and `filter -v` partition the records of a FASTQ and of a wrapped FASTA, order kept, bytes in the
    reference's record shape; the kept set = the records with an oracle match of any pattern (N filter as the CLI's
    default sets it)."""
    rng = random.Random(41)
    pats = [rand_seq(rng, 24) for _ in range(6)]
    k = 2
    (tmp_path / "p.txt").write_bytes(b"".join(p + b"\n" for p in pats))
    recs = []
    for i in range(120):
        tx = bytearray(rand_seq(rng, rng.randrange(60, 300)))
        if i % 3 != 2:
            ins = mutate(rng, pats[i % 6], i % 4)   # (3 edits: beyond k)
            if i % 2:
                ins = oracle.reverse_complement("iupac", ins)
            at = rng.randrange(0, len(tx) - 30)
            tx[at:at + len(ins)] = ins
        if i % 10 == 0:
            tx[5:25] = b"N" * 20
        recs.append((b"read%d some text" % i, bytes(tx), bytes(rng.choice(b"!#5AIJ") for _ in range(len(tx)))))
    fq = b"".join(b"@" + i + b"\n" + s + b"\n+\n" + q + b"\n" for i, s, q in recs)
    wrap = lambda s: b"\n".join(s[j:j + 60] for j in range(0, len(s), 60))
    fa = b"".join(b">" + i + b"\n" + wrap(s) + b"\n" for i, s, _ in recs)
    (tmp_path / "r.fq").write_bytes(fq)
    (tmp_path / "r.fa").write_bytes(fa)
    has = [any(oracle.search_modes("iupac", p, s, k, rc=True, max_n_frac=0.2) for p in pats) for _, s, _ in recs]
    assert 30 <= sum(has) <= 100
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(*argv):
        p = subprocess.run([sys.executable, "-m", "sassy_amd", "filter", "-l", str(tmp_path / "p.txt"), "-k", str(k)] + list(argv),
                           cwd=ROOT, env=env, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout

    for path, shape in ((str(tmp_path / "r.fq"), lambda i, s, q: b"@" + i + b"\n" + s + b"\n+\n" + q + b"\n"),
                        (str(tmp_path / "r.fa"), lambda i, s, q: b">" + i + b"\n" + s + b"\n")):
        kept, dropped = run(path), run("-v", path)
        assert kept == b"".join(shape(*r) for r, h in zip(recs, has) if h)
        assert dropped == b"".join(shape(*r) for r, h in zip(recs, has) if not h)
