"""search_all_alignments on the device against the CPU checker (tests/helpers/all_alignments_ref.py), order included."""
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import all_alignments_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

LETTERS = {"dna": b"ACGT", "iupac": b"ACGT", "ascii": b"ACGTacgt"}


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


def _mutate(rng, s: bytes, edits: int, letters: bytes) -> bytes:
    b = bytearray(s)
    for _ in range(edits):
        kind = rng.randrange(3)
        at = rng.randrange(len(b) + (kind == 1))
        if kind == 0 and b:
            b[at % len(b)] = rng.choice(letters)
        elif kind == 1:
            b.insert(at, rng.choice(letters))
        elif len(b) > 1:
            del b[at % len(b)]
    return bytes(b)


def _planted(rng, pattern: bytes, n: int, k: int, letters: bytes, plants: int, rc_plants: bool = False) -> bytes:
    t = bytearray(rng.choice(letters) for _ in range(n))
    for _ in range(plants):
        p = _mutate(rng, pattern, rng.randint(0, k), letters)
        if rc_plants and rng.random() < 0.5:
            import oracle
            p = oracle.reverse_complement("dna", p)
        at = rng.randint(0, max(0, n - len(p)))
        t[at:at + len(p)] = p
    return bytes(t[:n])


def _check(sassy, alphabet, pattern, text, k, rc, max_n_frac=None, only_best=False, searcher=None):
    s = searcher or sassy.Searcher(alphabet, rc=rc)
    if max_n_frac is not None:
        s.with_max_n_frac(max_n_frac)
    if only_best:
        s.only_best_match(True)
    got = ref.as_tuples(s.search_all_alignments(pattern, text, k))
    want = ref.search_all_alignments(alphabet, pattern, text, k, rc=rc, max_n_frac=max_n_frac, only_best=only_best)
    assert got == want, (alphabet, pattern, text[:200], k, rc, max_n_frac, only_best)
    return got


def test_golden_entries(sassy):
    with open(os.path.join(ROOT, "tests", "golden", "all_alignments.json")) as f:
        for e in json.load(f):
            got = _check(sassy, e["alphabet"], e["pattern"].encode(), e["text"].encode(), e["k"], e["rc"], e["max_n_frac"])
            ref.check_golden(e, got)


@pytest.mark.parametrize("alphabet", ["dna", "iupac", "ascii"])
def test_profiles_strands_lengths_and_k(sassy, alphabet):
    """k = 0..6, m in {4, 23, 32, 64, 100, 200}, both strands (Ascii: forward only), planted copies, matches at both
    ends of the text, texts shorter than m + k."""
    rng = random.Random({"dna": 1, "iupac": 2, "ascii": 3}[alphabet])
    L = LETTERS[alphabet]
    rcs = [False] if alphabet == "ascii" else [False, True]
    for m in (4, 23, 32, 64, 100, 200):
        for k in range(0, 7):
            if m == 4 and k > 3:
                continue
            if m >= 100 and k not in (0, 3, 6):
                continue
            pat = bytes(rng.choice(L) for _ in range(m))
            for rc in rcs:
                n = rng.choice([m + 3 * k + 40, 4 * m])
                text = _planted(rng, pat, n, k, L, 2)
                text = _mutate(rng, pat, rng.randint(0, k), L) + text + _mutate(rng, pat, rng.randint(0, k), L)
                _check(sassy, alphabet, pat, text, k, rc)
                short = _mutate(rng, pat, k, L)[: max(1, m + k - 2)]  # shorter than m + k
                _check(sassy, alphabet, pat, short, k, rc)


def test_n_runs_and_n_fraction(sassy):
    rng = random.Random(7)
    for alphabet in ("iupac",):  # ('N' is a letter of the Iupac profile only)
        for f in (1.0, 0.2):
            for m, k in ((8, 2), (23, 4)):
                pat = bytes(rng.choice(b"ACGT") for _ in range(m))
                t = bytearray(_planted(rng, pat, 400, k, b"ACGT", 4))
                for at in (30, 120, 250):
                    t[at:at + rng.randint(3, 12)] = b"N" * 12
                t[:6] = b"NNNNNN"
                text = bytes(t[:400]) + pat[: m - 2] + b"NN"
                _check(sassy, alphabet, pat, text, k, True, max_n_frac=f)


def test_only_best_match(sassy):
    rng = random.Random(11)
    for rc in (False, True):
        for k in (1, 3, 5):
            pat = bytes(rng.choice(b"ACGT") for _ in range(20))
            text = _planted(rng, pat, 600, k, b"ACGT", 5, rc_plants=True)
            _check(sassy, "dna", pat, text, k, rc, only_best=True)


def test_mib_text_with_plants(sassy):
    """1 MiB of random DNA, a plant every 2 KiB: thousands of end positions on both strands."""
    rng = random.Random(3)
    pat = bytes(rng.choice(b"ACGT") for _ in range(23))
    text = _planted(rng, pat, 1 << 20, 3, b"ACGT", 512, rc_plants=True)
    got = _check(sassy, "dna", pat, text, 3, True)
    assert sum(len(g) for g in got) > 1000


def test_low_complexity_many_batches(sassy):
    """A low-complexity text whose ends each have dozens of alignments, emitted through batches of at most 7 rows:
    equal to the checker and to the default batching, byte for byte."""
    rng = random.Random(5)
    unit = b"AAAAAAAAAAAC"
    text = (unit * 40)[:450] + bytes(rng.choice(b"ACGT") for _ in range(50))
    pat = b"AAAAAAAAAAAAAAA"
    s1 = sassy.Searcher("dna", rc=True)
    s2 = sassy.Searcher("dna", rc=True)
    s2.set_option("aa_batch", 7)
    a = _check(sassy, "dna", pat, text, 4, True, searcher=s1)
    b = _check(sassy, "dna", pat, text, 4, True, searcher=s2)
    assert a == b and sum(len(g) for g in a) > 500


def test_rc_equals_fwd_on_reverse_complement(sassy):
    """The reference's search_all_alignments_rc_fuzz: Rc alignments on T = Fwd alignments on RC(T) mapped back,
    cigars identical."""
    import oracle
    rng = random.Random(42)
    s_rc, s_fwd = sassy.Searcher("dna", rc=True), sassy.Searcher("dna", rc=False)
    for _ in range(200):
        plen = rng.randint(4, 20)
        pat = bytes(rng.choice(b"ACGT") for _ in range(plen))
        text = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(plen, plen + 10)))
        k = rng.randint(0, 3)
        n = len(text)
        rc = [x for g in s_rc.search_all_alignments(pat, text, k) for x in g if x.strand == "-"]
        fwd = [x for g in s_fwd.search_all_alignments(pat, oracle.reverse_complement("dna", text), k) for x in g]
        assert sorted((x.text_start, x.text_end, x.cost, x.cigar) for x in rc) == \
            sorted((n - x.text_end, n - x.text_start, x.cost, x.cigar) for x in fwd)


def test_anchors_are_search_all_ends_and_device_text(sassy):
    """Every group's anchor is an end position of search_all (Fwd: text_end, Rc: text_start), and a device tensor text
    gives the same groups as the bytes."""
    rng = random.Random(9)
    pat = bytes(rng.choice(b"ACGT") for _ in range(32))
    text = _planted(rng, pat, 20000, 3, b"ACGT", 20, rc_plants=True)
    s = sassy.Searcher("dna", rc=True)
    groups = s.search_all_alignments(pat, text, 3)
    ends = {(x.strand, x.text_end if x.strand == "+" else x.text_start) for x in s.search_all(pat, text, 3)}
    assert groups and all((g[0].strand, g[0].text_end if g[0].strand == "+" else g[0].text_start) in ends for g in groups)
    for g in groups:
        assert all(x.cost <= 3 and x.pattern_start == 0 and x.pattern_end == 32 for x in g)
    buf = sassy.DeviceBuffer(len(text) + 64)
    buf.upload(text)
    dev = DevText(buf.ptr, len(text))
    assert s.search_all_alignments(pat, dev, 3) == groups
    s.text_unchanged(True)
    assert s.search_all_alignments(pat, dev, 3) == groups


def test_overhang_refused_and_results_repeat(sassy):
    with pytest.raises(sassy.SassyHipError, match="-3"):
        sassy.Searcher("iupac", rc=False, alpha=0.5).search_all_alignments(b"ACGTACGT", b"ACGTACGTAA", 2)
    import ctypes as C
    rng = random.Random(13)
    pat = bytes(rng.choice(b"ACGT") for _ in range(16))
    text = _planted(rng, pat, 5000, 3, b"ACGT", 10, rc_plants=True)
    s = sassy.Searcher("dna", rc=True)
    L = sassy.lib()
    raw = []
    for _ in range(2):
        out = C.c_void_p()
        assert L.sassy_hip_search_all_alignments(s._h, pat, len(pat), C.c_char_p(text), len(text), 3, 0, C.byref(out)) == 0
        r = sassy.Result(out)
        raw.append((r.array.tobytes(), r.pool))
    assert raw[0] == raw[1] and len(raw[0][0]) > 0
