"""Searcher.search_hamming on the device against tests/helpers/hamming_ref.py (H in numpy, the relation from the oracle):
whole records compared for equality, order included."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import oracle  # noqa: E402
import hamming_ref as href  # noqa: E402

pytestmark = pytest.mark.gpu

LETTERS = {"dna": b"ACGT", "iupac": b"ACGTRYN", "ascii": b"abcdeAB _", "ascii_ci": b"abcdeABCDE[{_"}
PATTERN_LETTERS = {"dna": b"ACGT", "iupac": b"ACGTRN", "ascii": b"abcdeAB _", "ascii_ci": b"abcdeABCDE[{_"}
MS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)
# the driver's list (tests/c/hamming_step_driver.cc): every counter-plane boundary
K_LIST = (0, 1, 2, 3, 4, 7, 8, 15, 16, 63, 64, 254, 255, 256, 299, 300, 301)
TILE = 64 * 64        # bytes of text a wavefront owns (hamming_step.h: kHamTileBlocks blocks of 64)
GROUP = 4 * TILE      # ... a workgroup of four wavefronts


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


class DevText:
    """The parts of a device tensor the Python surface reads (data_ptr, numel, is_cuda, a 1-byte dtype)."""

    class _Byte:
        itemsize = 1

    dtype = _Byte()
    is_cuda = True

    def __init__(self, ptr: int, n: int):
        self._p, self._n = ptr, n

    def data_ptr(self):
        return self._p

    def numel(self):
        return self._n

    def is_contiguous(self):
        return True


def on_device(sassy, text: bytes):
    buf = sassy.DeviceBuffer(len(text) + 64)
    if text:
        buf.upload(text)
    return buf, DevText(buf.ptr, len(text))


def keys(matches):
    return [href.key(x) for x in matches]


def random_pattern(rng, profile, m):
    return bytes(rng.choice(PATTERN_LETTERS[profile]) for _ in range(m))


def planted_text(rng, profile, pattern, n, places, subs=(0, 1, 2, 3)):
    letters = LETTERS[profile]
    t = bytearray(rng.choice(letters) for _ in range(n))
    m = len(pattern)
    for i, at in enumerate(places):
        if at < 0 or at + m > n:
            continue
        w = bytearray(pattern)
        for _ in range(subs[i % len(subs)]):
            w[rng.randrange(m)] = rng.choice(letters)
        t[at:at + m] = w
    return bytes(t)


def shape_places(n, m):
    """Plants in the last byte of a block, of a wavefront's tile and of a workgroup's tiles, straddling those borders, and
    -- last, exact -- at start 0 and at n - m."""
    return [63, 127 * 64 + 63, TILE - 1, 2 * TILE - m // 2, GROUP - 1, GROUP - m // 2, 3 * GROUP - 1 - m // 3, 30000, 50001]


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("profile", ["dna", "iupac", "ascii", "ascii_ci"])
def test_all_shapes(sassy, profile, m):
    rng = random.Random(1000 * m + len(profile))
    n = 70001
    pattern = random_pattern(rng, profile, m)
    text = bytearray(planted_text(rng, profile, pattern, n, shape_places(n, m)))
    text[0:m] = pattern
    text[n - m:n] = pattern
    text = bytes(text)
    ks = sorted({0, 1, 3, m // 4})
    all_hits = href.expected(profile, pattern, text, max(ks))
    assert all_hits[0].text_start == 0 and all_hits[-1].text_start == n - m
    s = sassy.Searcher(profile, rc=False)
    buf, dev = on_device(sassy, text)
    for k in ks:
        want = keys(x for x in all_hits if x.cost <= k)
        assert keys(s.search_hamming(pattern, text, k)) == want, (profile, m, k, "host")
        assert keys(s.search_hamming(pattern, dev, k)) == want, (profile, m, k, "device")
    buf.free()


@pytest.mark.parametrize("profile", ["dna", "iupac", "ascii", "ascii_ci"])
def test_text_lengths(sassy, profile):
    rng = random.Random(77)
    s = sassy.Searcher(profile, rc=profile in ("dna", "iupac"))
    rc = profile in ("dna", "iupac")
    for m in (1, 5, 64, 65):
        pattern = random_pattern(rng, profile, m)
        for n in sorted({0, m - 1, m, m + 1, 63, 64, 65, 127, 128, 129}):
            text = planted_text(rng, profile, pattern, n, [0, n - m], subs=(1, 0))
            buf, dev = on_device(sassy, text)
            for k in (0, 2):
                want = keys(href.expected(profile, pattern, text, k, rc=rc))
                assert keys(s.search_hamming(pattern, text, k)) == want, (profile, m, n, k)
                assert keys(s.search_hamming(pattern, dev, k)) == want, (profile, m, n, k, "device")
                if n < m:
                    assert want == []
            buf.free()


def test_dense_k_at_least_m_and_forced_ranges(sassy):
    """k >= m reports every start, in order; again with the item list and the record block forced small, so that the driver
    cuts the text into several range launches and emits in many batches."""
    rng = random.Random(5)
    n, m = 20000, 5
    text = bytes(rng.choice(b"ACGT") for _ in range(n))
    pattern = b"ACGTA"
    s = sassy.Searcher("dna", rc=False)
    got = s.search_hamming(pattern, text, m)
    assert [x.text_start for x in got] == list(range(n - m + 1))
    want = keys(href.expected("dna", pattern, text, m))
    assert keys(got) == want
    assert keys(s.search_hamming(pattern, text, m + 7)) == want
    one = s.stats()["scan_launches"]
    s.set_option("hamming_items", 1).set_option("hamming_records", 100)
    assert keys(s.search_hamming(pattern, text, m)) == want
    assert s.stats()["scan_launches"] > max(4, one)
    # two patterns on both strands through the same small lists: the ranges' records come back in the contract's order
    s2 = sassy.Searcher("dna", rc=True)
    pats = [b"ACGTA", b"GGT"]
    want2 = keys(href.expected("dna", pats, text, 1, rc=True))
    assert keys(s2.search_hamming(pats, text, 1)) == want2
    s2.set_option("hamming_items", 300).set_option("hamming_records", 7)
    assert keys(s2.search_hamming(pats, text, 1)) == want2
    assert s2.stats()["scan_launches"] > 2


def test_every_value_of_h_at_every_threshold(sassy):
    """A text in which H takes every value 0 .. m (m = 300), searched at every k of the driver's list: saturation and the
    exactness of the threshold on the real kernel."""
    rng = random.Random(6)
    m = 300
    pattern = bytes(rng.choice(b"ACGT") for _ in range(m))
    other = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG"}
    parts = []
    for v in range(m + 1):
        w = bytearray(pattern)
        for j in rng.sample(range(m), v):
            w[j] = rng.choice(other[w[j]])
        parts.append(bytes(w) + bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 9))))
    text = b"".join(parts)
    h = href.mismatches("dna", pattern, text)
    assert set(range(m + 1)) <= set(h.tolist())
    s = sassy.Searcher("dna", rc=False)
    for k in K_LIST:
        if k <= 64:
            assert keys(s.search_hamming(pattern, text, k)) == keys(href.expected("dna", pattern, text, k)), k
        else:  # tens of thousands of hits: the columns, and the records at both ends
            r = s.search_hamming(pattern, text, k, as_result=True)
            _, _, starts, costs = href.expected_table("dna", pattern, text, k)
            arr = r.array
            assert np.array_equal(arr["text_start"].astype(np.int64), starts) and np.array_equal(arr["cost"].astype(np.int64), costs), k
            assert (arr["text_end"] - arr["text_start"] == m).all() and (arr["pattern_end"] == m).all()
            if k >= m:
                assert len(arr) == len(text) - m + 1
            lazy = r.lazy_matches
            head = href.expected("dna", pattern, text[:m + 40], k)
            assert keys(lazy[i] for i in range(len(head))) == keys(head), k


@pytest.mark.parametrize("profile", ["dna", "iupac"])
def test_both_strands(sassy, profile):
    rng = random.Random(8)
    s = sassy.Searcher(profile, rc=True)
    # a palindromic pattern: two records at one place, '+' first
    pal = b"AACGCGTT"
    assert oracle.reverse_complement(profile, pal) == pal
    text = bytearray(rng.choice(b"ACGT") for _ in range(3000))
    text[1000:1008] = pal
    got = s.search_hamming(pal, bytes(text), 0)
    at = [x for x in got if x.text_start == 1000]
    assert [(x.strand, x.cost, x.cigar) for x in at] == [("+", 0, "8="), ("-", 0, "8=")]
    assert keys(got) == keys(href.expected(profile, pal, bytes(text), 0, rc=True))
    # a mismatch at pattern position 1 of a minus-strand hit: at the cigar's start and at the span's end
    m = 20
    pattern = b"ACCGTTAGCATGGCATTCAG"
    changed = bytearray(pattern)
    changed[1] = ord("A")
    window = oracle.reverse_complement(profile, bytes(changed))
    text = bytearray(rng.choice(b"ACGT") for _ in range(5000))
    text[4095 - 7:4095 - 7 + m] = window
    text = bytes(text)
    got = s.search_hamming(pattern, text, 1)
    hit = [x for x in got if x.text_start == 4095 - 7]
    assert [(x.strand, x.cost, x.cigar) for x in hit] == [("-", 1, "1=1X18=")]
    scanned = oracle.reverse_complement(profile, pattern)
    assert text[hit[0].text_start + m - 2] != scanned[m - 2] and text[hit[0].text_start + 1] == scanned[1]
    assert keys(got) == keys(href.expected(profile, pattern, text, 1, rc=True))
    for mm in (1, 33, 64, 130):
        pattern = random_pattern(rng, profile, mm)
        t = bytearray(planted_text(rng, profile, pattern, 9000, [63, 4000, 8191 - mm // 2]))
        rcp = oracle.reverse_complement(profile, pattern)
        t[2000:2000 + mm] = rcp
        t[9000 - mm:] = rcp
        for k in (0, 2):
            assert keys(s.search_hamming(pattern, bytes(t), k)) == keys(href.expected(profile, pattern, bytes(t), k, rc=True)), (mm, k)


def test_multiple_patterns_share_a_call(sassy):
    """1, 2 and 17 patterns of mixed lengths in one call equal the per-pattern calls; with the patterns per launch forced
    down, too."""
    rng = random.Random(9)
    lengths = [1, 300, 2, 64, 65, 17, 128, 33, 5, 250, 31, 63, 129, 8, 100, 3, 20]
    for profile, rc in (("dna", True), ("ascii", False), ("iupac", True)):
        pats = [random_pattern(rng, profile, m) for m in lengths]
        text = bytearray(rng.choice(LETTERS[profile]) for _ in range(6000))
        for i, p in enumerate(pats):
            at = 300 * i + 17
            text[at:at + len(p)] = p
            text[at + len(p) // 2] = rng.choice(LETTERS[profile])
        text = bytes(text)
        s = sassy.Searcher(profile, rc=rc)
        k = 1
        single = [s.search_hamming(p, text, k) for p in pats]
        for count in (1, 2, 17):
            want = []
            for i in range(count):
                want += [href.key(x)[:0] + (i,) + href.key(x)[1:] for x in single[i]]
            assert keys(s.search_hamming(pats[:count], text, k)) == want, (profile, count)
        assert want == keys(href.expected(profile, pats, text, k, rc=rc))
        for batch in (1, 3):
            s.set_option("hamming_batch", batch)
            assert keys(s.search_hamming(pats, text, k)) == want, (profile, batch)
            assert s.stats()["scan_launches"] >= len(pats) * (2 if rc else 1) / batch
        s.set_option("hamming_batch", 0)


def test_ascii_pattern_set_beyond_the_slot_count(sassy):
    """Three patterns of 40 distinct bytes each, 120 together: more than the 64 slots of one launch."""
    rng = random.Random(10)
    pats = [bytes(range(10, 50)), bytes(range(60, 100)), bytes(range(130, 170)) + b"\x00\xff"]
    text = bytearray(rng.randrange(256) for _ in range(13000))
    for i, p in enumerate(pats):
        for at in (100 + 1000 * i, (i + 1) * TILE - 20, 8400 + 300 * i):
            text[at:at + len(p)] = p
            text[at + 3 + i] ^= 0x55
    text = bytes(text)
    for profile in ("ascii", "ascii_ci"):
        s = sassy.Searcher(profile, rc=False)
        for k in (0, 1, 5):
            want = keys(href.expected(profile, pats, text, k))
            assert len(want) >= (0 if k == 0 else 9)
            assert keys(s.search_hamming(pats, text, k)) == want, (profile, k)
        assert s.stats()["scan_launches"] >= 2
    # 64 distinct bytes in one pattern: one launch with every slot in use
    p64 = bytes(range(100, 164))
    t = bytearray(text)
    t[5000:5064] = p64
    t[5010] = 0
    s = sassy.Searcher("ascii", rc=False)
    assert keys(s.search_hamming(p64, bytes(t), 2)) == keys(href.expected("ascii", p64, bytes(t), 2))
    assert [x.text_start for x in s.search_hamming(p64, bytes(t), 2)] == [5000]


@pytest.mark.parametrize("frac", [0.0, 0.1, 0.2, 0.3, 0.5, None])
def test_max_n_frac(sassy, frac):
    """Iupac text with runs of N of every length up to 2 m; m = 10 makes 2 and 3 N the equality cases of 0.2 and 0.3."""
    rng = random.Random(12)
    m = 10
    pattern = b"ACGTTGCAAC"
    parts = []
    for run in range(1, 2 * m + 1):
        parts.append(bytes(rng.choice(b"ACGT") for _ in range(7)) + pattern[:5] + b"N" * run + pattern[5:] + bytes(rng.choice(b"ACGTn") for _ in range(9)))
    text = b"".join(parts) + pattern
    for rc in (False, True):
        s = sassy.Searcher("iupac", rc=rc).with_max_n_frac(frac)
        for k in (0, 3, 10):
            want = href.expected("iupac", pattern, text, k, rc=rc, max_n_frac=frac)
            assert keys(s.search_hamming(pattern, text, k)) == keys(want), (frac, rc, k)
    if frac in (0.2, 0.3):
        kept = {text[x.text_start:x.text_end].upper().count(b"N") for x in href.expected("iupac", pattern, text, 10, max_n_frac=frac)}
        assert max(kept) == round(frac * m)


def test_a_long_run_of_n_takes_no_list_space(sassy):
    """1 MiB of N under an Iupac searcher: every start is a Hamming hit, and the N filter drops them on the device before
    they reach the item list."""
    pattern = b"ACGTTGCAACGGATCAGTCA"
    text = b"N" * (1 << 20) + b"ACGT" * 5 + pattern + b"TTTT"
    s = sassy.Searcher("iupac", rc=False).with_max_n_frac(0.2)
    s.set_option("hamming_items", 64)
    got = s.search_hamming(pattern, text, 3)
    want = href.expected("iupac", pattern, text, 3, max_n_frac=0.2)
    assert keys(got) == keys(want) and len(want) >= 1
    st = s.stats()
    assert st["scan_launches"] == 1 and st["hit_blocks"] <= 4, st
    # without the filter the same text is dense
    s2 = sassy.Searcher("iupac", rc=False).with_max_n_frac(None)
    r = s2.search_hamming(pattern, text, 3, without_trace=True, as_result=True)
    assert len(r.array) >= (1 << 20) - len(pattern) + 1  # (every window that lies inside the run)


def test_without_trace_and_ties_to_the_engine(sassy):
    rng = random.Random(14)
    for profile in ("dna", "ascii"):
        m = 24
        pattern = random_pattern(rng, profile, m)
        text = planted_text(rng, profile, pattern, 30000, [63, 5000, 8191, 16383, 29000], subs=(0, 1, 2, 3, 0))
        s = sassy.Searcher(profile, rc=False)
        full = s.search_hamming(pattern, text, 3)
        bare = s.search_hamming(pattern, text, 3, without_trace=True)
        assert keys(bare) == keys(href.expected(profile, pattern, text, 3, without_trace=True))
        assert [href.key(x)[:-1] for x in full] == [href.key(x)[:-1] for x in bare] and all(x.cigar == "" for x in bare)
        assert len(full) >= 5
        # k = 0: the spans of this library's own search_all
        spans = sorted({(x.text_start, x.text_end) for x in s.search_all(pattern, text, 0)})
        assert [(x.text_start, x.text_end) for x in s.search_hamming(pattern, text, 0)] == spans and spans
        # every hit: the edit distance ending there is no larger
        row = oracle.last_row(profile, pattern, text)
        assert all(row[x.text_end] <= x.cost for x in full)
        assert s.stats()["filtered"] == 7 and s.stats()["scan_ms"] > 0


def test_large_text_generated_on_the_device(sassy):
    """40 MiB: more workgroups than the device holds at once (a workgroup takes 4 tiles of 4 KiB; 256 CUs hold at most 8
    workgroups of 256 threads each, 32 MiB of text)."""
    n = 40 * (1 << 20) + 1234
    assert n > 256 * 8 * GROUP
    m, k = 12, 1
    pattern = b"ACGGTCATTGCA"
    buf = sassy.DeviceBuffer(n + 64)
    sassy.generate_dna(buf.ptr, n, 4242)
    for at in (0, TILE - 1, GROUP - 5, 17 * GROUP - 1, 33 * (1 << 20) + 63, n - m):
        buf.upload(pattern, at)
    t = buf.download_into(np.empty(n, dtype=np.uint8))
    codes = (t >> 1) & 3
    h = np.zeros(n - m + 1, dtype=np.uint8)
    for j, p in enumerate(pattern):
        h += codes[j:j + n - m + 1] != ((p >> 1) & 3)
    starts = np.nonzero(h <= k)[0]
    s = sassy.Searcher("dna", rc=False)
    r = s.search_hamming(pattern, DevText(buf.ptr, n), k, as_result=True)
    arr = r.array
    assert np.array_equal(arr["text_start"].astype(np.int64), starts) and np.array_equal(arr["cost"], h[starts].astype(np.int32))
    assert len(starts) >= 6 and starts[0] == 0 and starts[-1] == n - m
    for sample in (r.lazy_matches[0], r.lazy_matches[len(arr) // 2], r.lazy_matches[len(arr) - 1]):
        exp = href.expected("dna", pattern, bytes(t[sample.text_start:sample.text_end]), k)[0]
        assert (sample.text_end - sample.text_start, sample.cost, sample.cigar, sample.strand) == (m, exp.cost, exp.cigar, "+")
    buf.free()


def test_random_slice(sassy):
    """A seeded slice over all of the above dimensions at once."""
    rng = random.Random(20261018)
    for it in range(70):
        profile = rng.choice(["dna", "iupac", "ascii", "ascii_ci"])
        rc = profile in ("dna", "iupac") and rng.random() < 0.5
        n = rng.choice([0, 1, 63, 64, 65, 200, 4095, 4096, 4097, 9000, 20000])
        pats = []
        for _ in range(rng.choice([1, 1, 2, 3])):
            m = rng.choice([1, 2, 3, 8, 20, 31, 32, 33, 63, 64, 65, 100, 128, 129, 300])
            pats.append(random_pattern(rng, profile, m))
        k = rng.choice([0, 1, 2, 3, 4, 7, 8, 15, 16, 63, 64])
        if n >= 9000 and k >= min(len(p) for p in pats) // 2:
            k = rng.choice([0, 1, 2])  # (keep the dense cases for the small texts)
        text = bytearray(rng.choice(LETTERS[profile]) for _ in range(n))
        for p in pats:
            for _ in range(3):
                if n >= len(p):
                    at = rng.choice([0, n - len(p), rng.randrange(0, n - len(p) + 1), max(0, min(n - len(p), 4096 - rng.randrange(1, 70)))])
                    w = bytearray(p if not (rc and rng.random() < 0.5) else oracle.reverse_complement(profile, p))
                    for _ in range(rng.randrange(0, 4)):
                        w[rng.randrange(len(w))] = rng.choice(LETTERS[profile])
                    text[at:at + len(p)] = w
        text = bytes(text)
        frac = rng.choice([None, None, 0.0, 0.2, 0.5]) if profile == "iupac" else None
        wt = rng.random() < 0.25
        s = sassy.Searcher(profile, rc=rc).with_max_n_frac(frac)
        if rng.random() < 0.3:
            s.set_option("hamming_items", rng.choice([1, 200])).set_option("hamming_records", rng.choice([3, 1000]))
            s.set_option("hamming_batch", rng.choice([0, 1, 2]))
        where = text
        buf = None
        if rng.random() < 0.4:
            buf, where = on_device(sassy, text)
        got = keys(s.search_hamming(pats if len(pats) > 1 or rng.random() < 0.5 else pats[0], where, k, without_trace=wt))
        want = keys(href.expected(profile, pats, text, k, rc=rc, max_n_frac=frac, without_trace=wt))
        assert got == want, (it, profile, rc, n, [len(p) for p in pats], k, frac, wt)
        if buf is not None:
            buf.free()
