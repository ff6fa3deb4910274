"""The catalogue of calls for the call-order tests (tests/test_gpu_call_order.py, tests/test_call_catalogue_cpu.py): every
public entry point of sassy_amd.Searcher as one or more entries, each with the call (`run`, on a device) and its expected
value (`expect`, on the host), both in ONE canonical, hashable form so that a test compares them with `==` and nothing else.

Importing this module needs no device.  The expectations come from what the project already has -- oracle.search,
search_modes, search_overhang, search_encoded and tests/helpers/*_ref.py -- and this file holds no second definition of any
operation: it only builds inputs, calls those, and brings both sides into the canonical form.

Searcher kinds.  A searcher has a fixed alphabet, strand setting and alpha, so the catalogue is run once per kind:
  dna, dna-rc, iupac, iupac-rc   the nucleotide searchers, everything applies
  iupac-alpha                    Searcher("iupac", rc=False, alpha=0.5): the overhang searcher -- only such a searcher uploads
                                 the overhang delta table, and the Hamming / set / all-alignment calls refuse it
  ascii, ascii_ci                no reverse complement: the text-search side (class patterns live here only)
An entry lists the kinds it applies to; a call that cannot run for a kind is not in that kind's list.

Canonical forms.
  matches   the sorted tuple of (text_idx, pattern_idx, text_start, text_end, pattern_start, pattern_end, cost, strand, cigar)
            -- the fields and order of best_matches_ref.record and hamming_many_ref.key_matches; a result of more than
            BIG_ROWS records: ("rows", n, sha1 of the same records, sorted, as columns) so that a dense result costs numpy time
  arrays    (dtype.str, shape, tobytes()); structured records field by field (their pad bytes are not part of the contract)
  handles   everything tests/test_gpu_merge_pairs.py::compare looks at: the six record columns, longest, text_bytes, whether
            the pointers are set, the text and quality buffers byte for byte, the block table

The calls that take ONE text of the Hamming family (search_hamming, hamming_counts, hamming_amplicons) run on a host text and on
a resident one; the batch calls on a list and on a DeviceReads.  The set calls' big sibling is hamming_pairs at n = 3 000 (the
pair families share d_pairs_*; the edit distances of 9e6 pairs would cost the host expectation more than all the rest).

Inputs (fixed seeds; all under 1 MiB).  T1: 6 KiB of random DNA with five planted near-matches of P20 and plants of the other
patterns.  T2: 40 KiB of low-complexity text.  The seeded route of search_encoded_patterns: the smallest input that takes it
by the library's own estimate (c_abi.hip: seeded_estimate against the tiled scan's) with one text and 20-mers at k = 2 needs
n_patterns x text_len of about 5e8; the entry uses SEEDED_PATTERNS = 2048 patterns over SEEDED_TEXT = 320 KiB (text_len must
exceed 240 KiB at 2048 patterns), well under 1 MiB.
"""
import collections
import hashlib
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402

import all_alignments_ref as aref  # noqa: E402
import amplicon_ref  # noqa: E402
import best_matches_ref as bref  # noqa: E402
import clusters_ref  # noqa: E402
import edit_pairs_ref as eref  # noqa: E402
import fasta_ref  # noqa: E402
import fastq_ref  # noqa: E402
import hamming_counts_ref as hcref  # noqa: E402
import hamming_many_ref as hmref  # noqa: E402
import hamming_pairs_ref as pref  # noqa: E402
import hamming_ref as href  # noqa: E402
import line_spans_ref as lref  # noqa: E402
import merge_pairs_ref as mref  # noqa: E402
import read_overlaps_ref as oref  # noqa: E402
import umi_groups_ref as uref  # noqa: E402
from prose_text import fold  # noqa: E402
from trace_shapes import mapped  # noqa: E402

THREADS = 16
BIG_ROWS = 4096

Kind = collections.namedtuple("Kind", "id alphabet rc alpha")
KINDS = [Kind("dna", "dna", False, None), Kind("dna-rc", "dna", True, None), Kind("iupac", "iupac", False, None),
         Kind("iupac-rc", "iupac", True, None), Kind("iupac-alpha", "iupac", False, 0.5), Kind("ascii", "ascii", False, None),
         Kind("ascii_ci", "ascii_ci", False, None)]
KIND = {k.id: k for k in KINDS}
NUC = ("dna", "dna-rc", "iupac", "iupac-rc")
TEXTY = ("ascii", "ascii_ci")
PLAIN = NUC + TEXTY           # every kind but the overhang searcher
ALL = PLAIN + ("iupac-alpha",)
WITH_N = ("iupac", "iupac-rc") + TEXTY   # kinds whose text may hold an N (a dna searcher's text is A C G T only)


def make_searcher(sassy, kind):
    return sassy.Searcher(kind.alphabet, rc=kind.rc, alpha=kind.alpha)


# ================================================================ inputs
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _dna(rng, n):
    return bytes(rng.choice(_ACGT, n).astype(np.uint8)) if n else b""


def _subs(seq, where):
    """seq with the base at each position of `where` replaced by the next one of A -> C -> G -> T -> A"""
    nxt = {65: 67, 67: 71, 71: 84, 84: 65}
    s = bytearray(seq)
    for i in where:
        s[i] = nxt[s[i]]
    return bytes(s)


def _put(buf, at, seq):
    buf[at:at + len(seq)] = seq


SEEDED_PATTERNS = 2048
SEEDED_TEXT = 320 * 1024


class Data:
    """Every host input, made once (fixed seeds)."""

    def __init__(self):
        rng = np.random.default_rng(20261021)
        self.p20 = b"ACGTTGCAAGCTCAGGTCAT"
        self.p20b = b"TGACCATGGTACTTCAGGCA"      # the same length, other bytes: the upload cache's probe
        self.p12 = b"GATTACAGGCTC"
        self.p15 = b"CCGTATAGCTAAGGT"            # k = 2: five-row pieces, the streaming scan without a filter
        self.p300 = _dna(rng, 300)
        t1 = bytearray(_dna(rng, 6144))
        # five near-matches of P20: exact, one and two substitutions, a deletion, an insertion with a substitution
        for at, v in ((200, self.p20), (1400, _subs(self.p20, [7])), (3700, _subs(self.p20, [3, 15])), (4900, self.p20[:9] + self.p20[10:]),
                      (5800, _subs(self.p20[:12] + b"T" + self.p20[12:], [2]))):
            _put(t1, at, v)
        _put(t1, 3400, _subs(self.p20, [1, 8, 17]))   # ... and a relative at three substitutions: k = 3 finds it, k = 2 does not
        for at, v in ((700, self.p20b), (4300, _subs(self.p20b, [5, 11]))):
            _put(t1, at, v)
        for at, v in ((1000, self.p12), (5200, _subs(self.p12, [6]))):
            _put(t1, at, v)
        for at, v in ((1700, _subs(self.p15, [4])), (5500, _subs(self.p15, [1, 9]))):
            _put(t1, at, v)
        _put(t1, 2200, _subs(self.p300, [10, 60, 110, 160, 210, 260]))
        self.t1 = bytes(t1)
        # the text-search kinds see it in mixed case: the second half is lower case (ascii: no match there; ascii_ci: all)
        self.t1_case = self.t1[:3072] + self.t1[3072:].lower()
        # ... with X / Y at rows 4, 10, 16 of the plants at 200 and 1400: the class pattern's text
        tc = bytearray(self.t1_case)
        for at, letters in ((200, b"YXY"), (1400, b"XYX")):
            for row, c in zip((4, 10, 16), letters):
                tc[at + row] = c
        self.t1_class = bytes(tc)
        # T1 with the exact plant at 200 carrying two N: the N filter's probe
        tn = bytearray(self.t1)
        tn[205], tn[213] = ord("N"), ord("N")
        self.tn = bytes(tn)
        self.tn_case = bytes(tn[:3072]) + bytes(tn[3072:]).lower()
        # ... with a newline about every 80 bytes (never inside P20's first plant): the line calls
        tl = bytearray(self.t1)
        for at in range(79, len(tl), 83):
            if not 190 <= at <= 230:
                tl[at] = 10
        self.tl = bytes(tl)
        self.tl_case = bytes(tl[:3072]) + bytes(tl[3072:]).lower()
        # the "same pointer, new contents" pair: T1 and T1 with its halves swapped
        self.t1_swapped = self.t1[3072:] + self.t1[:3072]
        # T2: low complexity -- poly-A stretches, microsatellites -- between random stretches
        parts = [_dna(rng, 4000), b"A" * 3000, _dna(rng, 5000), b"CAG" * 200, _dna(rng, 6000), b"A" * 1500, _dna(rng, 4000), b"AT" * 300,
                 _dna(rng, 7000), b"A" * 700, b"GATA" * 100]
        t2 = bytearray(b"".join(parts))
        t2 += _dna(rng, 40960 - len(t2))
        _put(t2, 1000, self.p20)
        _put(t2, 12500, _subs(self.p20, [4, 14]))
        self.t2 = bytes(t2)
        self.pmicro = b"CAGCAGCAGCAGCAGCAGCA"
        # the overhang searcher's text: P20 hangs over its start by 6 rows and over its end by 7
        self.tov = self.p20[6:] + _dna(rng, 900) + _subs(self.p20, [9]) + _dna(rng, 900) + self.p20[:13]
        # many texts: 30 of 50 .. 300 bytes; four 20-mers; plants of them
        self.pats4 = [self.p20, self.p20b, b"GGATCCTTAAGCATGCAATG", b"CATGATTGACCTGAACGTCA"]
        lens = [50, 300, 64, 65, 63, 128, 129] + [int(x) for x in rng.integers(50, 301, 23)]
        texts = []
        for i, n in enumerate(lens):
            t = bytearray(_dna(rng, n))
            p = self.pats4[i % 4]
            if i % 5 != 4:
                _put(t, (7 * i) % (n - 20), _subs(p, [i % 20][:i % 2]))
            if i % 6 == 1:
                _put(t, n - 20, oref.revcomp("dna", _subs(self.pats4[(i + 1) % 4], [5])))
            texts.append(bytes(t))
        self.texts30 = texts
        self.texts30_case = [t.lower() if i % 3 == 2 else t for i, t in enumerate(texts)]
        # search_encoded, tiled route: eight 20-mers, six of them cut from T1
        self.pats8 = [self.p20, self.p20b] + [self.t1[2600 + 100 * i:2620 + 100 * i] for i in range(6)]
        # ... seeded route (see the docstring): 2048 20-mers, 64 of them cut from the text
        self.seeded_text = _dna(rng, SEEDED_TEXT)
        self.seeded_pats = [self.seeded_text[5000 * i + 11:5000 * i + 31] for i in range(64)] + \
                           [_dna(rng, 20) for _ in range(SEEDED_PATTERNS - 64)]
        # Hamming: patterns of mixed lengths; primer pairs 300 apart in T1
        self.hpats = [self.p20, self.p12, self.p15]
        self.primers = [(self.t1[3000:3018], oref.revcomp("dna", self.t1[3282:3300])), (self.p20[:16], oref.revcomp("dna", self.p20b[-16:]))]
        # sets: n = 200, m = 16 -- 40 families of five relatives
        base = rng.choice(_ACGT, (40, 16)).astype(np.uint8)
        rows = []
        for f in range(40):
            for r in range(5):
                row = base[f].copy()
                for e in range(r % 3):
                    row[(3 * r + 5 * e + f) % 16] = _ACGT[(int(np.flatnonzero(_ACGT == row[(3 * r + 5 * e + f) % 16])[0]) + 1 + e) % 4]
                if r == 4:
                    row = np.concatenate([row[1:], row[:1]])  # a shift: edit distance 2, far in Hamming distance
                rows.append(row)
        self.set_a = np.ascontiguousarray(np.stack(rows))
        self.set_b = np.ascontiguousarray(np.concatenate([base[:30], rng.choice(_ACGT, (20, 16)).astype(np.uint8)]))
        # UMIs: 200 reads over 30 distinct sequences with skewed counts, neighbours among them
        umi = rng.choice(_ACGT, (30, 16)).astype(np.uint8)
        for i in range(1, 30, 2):
            umi[i] = umi[i - 1]
            umi[i, i % 16] = _ACGT[(int(np.flatnonzero(_ACGT == umi[i, i % 16])[0]) + 1) % 4]
        draw = rng.choice(30, 200, p=np.array([8.0 if i % 2 == 0 else 2.0 for i in range(30)]) / 150.0)
        self.umis = np.ascontiguousarray(umi[draw])
        # the big siblings
        self.big_text = b"A" * 70000
        self.big_pat = b"A" * 20
        self.big_ham_text = b"A" * 20011      # 20 000 starts of A x 12
        self.big_ham_pat = b"A" * 12
        big_base = rng.choice(_ACGT, (1000, 16)).astype(np.uint8)
        big = big_base[rng.integers(0, 1000, 3000)].copy()
        flip = rng.random(3000) < 0.3
        col = rng.integers(0, 16, 3000)
        big[flip, col[flip]] = _ACGT[rng.integers(0, 4, int(flip.sum()))]
        self.set_big = np.ascontiguousarray(big)
        # reads: FASTQ of ten reads (ids, CRLF in one record); FASTA of three records, the second is T1 wrapped at 70
        seqs = [self.texts30[i] for i in range(9)] + [b""]
        self.fastq = b"".join(b"@read%d some text\n%s\n+\n%s\n" % (i, s, bytes(rng.integers(33, 75, len(s)).astype(np.uint8)))
                              for i, s in enumerate(seqs)).replace(b"@read3 some text\n", b"@read3 some text\r\n")
        self.fasta = b">first record\n" + self.texts30[1] + b"\n>t1 wrapped\r\n" + \
                     b"\n".join(self.t1[i:i + 70] for i in range(0, len(self.t1), 70)) + b"\n>last\n" + self.texts30[5] + b"\n"
        # paired reads: the `batch` fixture of tests/test_gpu_merge_pairs.py (70 pairs: overlaps, read-throughs, empty reads, none)
        prng = np.random.default_rng(25)
        rand_seq = lambda n: bytes(prng.choice(_ACGT, n).astype(np.uint8)) if n else b""  # noqa: E731
        r1s, r2s = [], []
        for i in range(70):
            la, lb = int(prng.integers(30, 200)), int(prng.integers(30, 200))
            d = int(prng.integers(0, la - 15)) if i % 3 else -int(prng.integers(1, lb - 15))
            a, r2 = oref.planted_pair(prng, "dna", la, lb, d, subs=i % 3)
            if i % 10 == 9:
                a, r2 = (b"", r2) if i % 20 == 9 else (rand_seq(la), oref.revcomp("dna", rand_seq(lb)))
            r1s.append(a)
            r2s.append(r2)
        qual = lambda s: bytes(prng.integers(33, 75, len(s)).astype(np.uint8))  # noqa: E731
        self.pairs1, self.pairs2 = [(s, qual(s)) for s in r1s], [(s, qual(s)) for s in r2s]
        self.pair_call = (10, 5, 200)   # min_overlap, k, max_permille
        # ... the big sibling: 1 100 pairs, mostly short, the longest read 512 bytes
        b1, b2 = [], []
        for i in range(1100):
            la, lb = (512, 512) if i in (7, 600, 1099) else (int(prng.integers(30, 80)), int(prng.integers(30, 80)))
            a, r2 = oref.planted_pair(prng, "dna", la, lb, int(prng.integers(0, la - 12)), subs=i % 2)
            b1.append(a)
            b2.append(r2)
        self.big_r1, self.big_r2 = b1, b2


_DATA = None


def data():
    global _DATA
    if _DATA is None:
        _DATA = Data()
    return _DATA


# ================================================================ canonical forms
def rec(m, text_idx=0):
    """one match as the tuple the canonical form sorts: best_matches_ref.record's fields and order"""
    return bref.record(m, text_idx)


def _rows_digest(cols, cigars):
    """("rows", n, sha1): cols a (n, 8) uint64 array in rec()'s order without the cigar, strand 0 / 1; cigars an 'S' array"""
    order = np.lexsort((cigars,) + tuple(cols[:, j] for j in range(7, -1, -1)))
    h = hashlib.sha1(np.ascontiguousarray(cols[order]).tobytes())
    h.update(np.ascontiguousarray(cigars[order]).tobytes())
    return ("rows", len(cols), h.hexdigest())


def canon_matches(matches, text_idx=None):
    """Match objects (sassy_amd.Match with its text_idx, or oracle.Match with the one given) -> the canonical form"""
    recs = [rec(m, getattr(m, "text_idx", 0) if text_idx is None else text_idx) for m in matches]
    return canon_records(recs)


def canon_records(recs):
    if len(recs) <= BIG_ROWS:
        return tuple(sorted(recs))
    cols = np.array([r[:7] + (1 if r[7] == "-" else 0,) for r in recs], dtype=np.uint64)
    width = max(len(r[8]) for r in recs)
    return _rows_digest(cols, np.array([r[8].encode() for r in recs], dtype="S%d" % max(1, width)))


def peek(sassy, r):
    """(array, pool) of a Result WITHOUT letting go of its C records: a result that is kept alive stays adopted"""
    if not getattr(r, "_h", None):
        return r.array, r.pool
    L = sassy.lib()
    n = len(r)
    arr = np.frombuffer(sassy._bytes_at(L.sassy_hip_result_matches(r._h), n * 64), dtype=sassy.match_dtype())
    pool = sassy._bytes_at(L.sassy_hip_result_cigars(r._h), L.sassy_hip_result_cigars_len(r._h))
    return arr, pool


def canon_result(sassy, r):
    """a Result -> the canonical form of its records (read in place: see peek)"""
    arr, pool = peek(sassy, r)
    n = len(arr)
    if n <= BIG_ROWS:
        return tuple(sorted(rec(m, m.text_idx) for m in sassy.matches_from_array(arr, pool)))
    cols = np.stack([arr[f].astype(np.uint64) for f in ("text_idx", "pattern_idx", "text_start", "text_end", "pattern_start", "pattern_end", "cost",
                                                       "strand")], axis=1)
    off, ln = arr["cigar_off"].astype(np.int64), arr["cigar_len"].astype(np.int64)
    width = max(1, int(ln.max()))
    p = np.frombuffer(pool + bytes(width), dtype=np.uint8)
    grid = p[off[:, None] + np.arange(width)[None, :]] * (np.arange(width)[None, :] < ln[:, None])
    return _rows_digest(cols, np.ascontiguousarray(grid.astype(np.uint8)).view("S%d" % width).ravel())


def canon_results(sassy, results):
    return tuple(canon_result(sassy, r) for r in results)


def canon_array(a):
    a = np.ascontiguousarray(a)
    return (a.dtype.str, a.shape, a.tobytes())


def canon_arrays(arrays):
    return tuple(canon_array(a) for a in arrays)


def canon_fields(a, fields):
    """a structured array field by field (its pad bytes are not part of the contract): (name, dtype.str, shape, bytes) each"""
    return tuple((f,) + canon_array(a[f]) for f in fields)


PAIR_FIELDS = (("a_idx", "<u4"), ("b_idx", "<u4"), ("cost", "u1"), ("strand", "u1"))
AMPLICON_FIELDS = (("start", "<u8"), ("end", "<u8"), ("pair_idx", "<u4"), ("strand", "u1"), ("fwd_cost", "u1"), ("rev_cost", "u1"))
OVERLAP_FIELDS = (("offset", "<i4"), ("overlap", "<u4"), ("mismatches", "<u4"), ("n_accepted", "<u4"))
SPAN_FIELDS = (("line_no", "<u8"), ("last_line_no", "<u8"), ("line_start", "<u8"), ("line_end", "<u8"))


def canon_struct(a, spec):
    return tuple((f,) + canon_array(np.asarray(a[f]).astype(dt)) for f, dt in spec)


def canon_handle(h):
    """everything tests/test_gpu_merge_pairs.py::compare looks at of a read batch with kept qualities"""
    return (len(h),) + tuple(canon_array(np.asarray(c).astype(np.uint64)) for c in (h.seq_starts, h.seq_lens, h.qual_starts, h.qual_lens, h.id_starts,
                                                                                   h.id_lens)) + \
        (int(h.longest), int(h.text_bytes), bool(h.ptr), bool(h.qual_ptr), bytes(h.download_text()), bytes(h.download_quality_text()),
         canon_array(h.download_rem()))


def expected_handle(seqs, quals):
    """the same of the helper's merged sequences and qualities (merge_pairs_ref.layout_of, rem_of)"""
    starts, lens, text = mref.layout_of(seqs)
    qual = mref.layout_of(quals)[2]
    zero = np.zeros(len(seqs), dtype=np.uint64)
    return (len(seqs),) + tuple(canon_array(np.asarray(c).astype(np.uint64)) for c in (starts, lens, starts, lens, zero, zero)) + \
        (int(lens.max()) if len(lens) else 0, int(text.size), True, True, text.tobytes(), qual.tobytes(), canon_array(mref.rem_of(starts, lens)))


# ================================================================ the fixtures of one kind
class Fixtures:
    """The inputs as one kind sees them, the oracle under that kind's settings, and a memo of the expectations.  `dev`: the
    device-side objects (DeviceSide), set by the GPU tests only."""

    def __init__(self, kind, dev=None):
        self.kind, self.d, self.dev = kind, data(), dev
        self.profile, self.rc, self.alpha = kind.alphabet, kind.rc, kind.alpha
        self.texty = kind.id in TEXTY
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    # --- inputs that differ between the kinds
    @property
    def t1(self):
        return self.d.t1_case if self.texty else self.d.t1

    @property
    def tn(self):
        return self.d.tn_case if self.texty else self.d.tn

    @property
    def tl(self):
        # (a dna searcher's text holds A C G T only -- the oracle's traceback refuses other bytes, as the reference's would --,
        # so its line calls see the one line of T1)
        return self.d.tl_case if self.texty else self.d.t1 if self.profile == "dna" else self.d.tl

    @property
    def texts30(self):
        return self.d.texts30_case if self.texty else self.d.texts30

    # --- the oracle under this kind's settings
    def _fold(self, x):
        return fold(x) if self.profile == "ascii_ci" else bytes(x)

    @property
    def oprofile(self):
        return "ascii" if self.profile == "ascii_ci" else self.profile

    def search(self, pattern, text, k, all_minima=False, rc=None, max_overhang=None, **modes):
        """oracle matches of one pattern in one text: plain, with reporting modes (search_modes), or with overhang"""
        rc = self.rc if rc is None else rc
        p, t = self._fold(pattern), self._fold(text)
        if max_overhang is not None:
            assert self.alpha is not None and not rc and not modes
            return oracle.search_overhang(self.oprofile, p, t, k, self.alpha, rc=False, all_minima=all_minima, max_overhang=max_overhang)
        if modes or self.alpha is not None:
            return oracle.search_modes(self.oprofile, p, t, k, rc=rc, all_minima=all_minima, alpha=self.alpha, **modes)
        return oracle.search(self.oprofile, p, t, k, rc=rc, all_minima=all_minima)

    def pair_matches(self, patterns, texts, k):
        """{(p, t): oracle matches} of every pattern in every text, once"""
        def build():
            return {(pi, ti): self.search(p, t, k) for pi, p in enumerate(patterns) for ti, t in enumerate(texts)}
        return self.memo(("pairs", tuple(patterns), tuple(texts), k), build)


class DeviceSide:
    """What lives on the device for the whole test module and is shared by every searcher: resident texts, the read batches.
    Nothing here belongs to a searcher (that is the point: one DeviceReads serves a dna searcher, then an iupac one)."""

    def __init__(self, sassy):
        self.sassy, d = sassy, data()
        self._texts, self._buffers = {}, []
        self.swap = sassy.DeviceBuffer(len(d.t1) + 256)
        self.reads30 = sassy.DeviceReads.from_sequences(d.texts30)
        self.h1 = sassy.DeviceReads.from_sequences([x[0] for x in d.pairs1], [x[1] for x in d.pairs1])
        self.h2 = sassy.DeviceReads.from_sequences([x[0] for x in d.pairs2], [x[1] for x in d.pairs2])
        self.plain1 = sassy.DeviceReads.from_sequences([x[0] for x in d.pairs1])
        self.big1 = sassy.DeviceReads.from_sequences(d.big_r1)
        self.big2 = sassy.DeviceReads.from_sequences(d.big_r2)
        self.long1 = sassy.DeviceReads.from_sequences([b"A" * 513, b"ACGT"])
        self.short2 = sassy.DeviceReads.from_sequences([b"ACGTACGTACGT", b"ACGT"])

    def resident(self, text):
        """`text` on the device (uploaded once): a DeviceText"""
        if text not in self._texts:
            buf = self.sassy.DeviceBuffer(len(text) + 256)
            buf.upload(text)
            self._buffers.append(buf)
            self._texts[text] = self.sassy.DeviceText(buf.ptr, len(text), owner=buf)
        return self._texts[text]

    def close(self):
        for h in (self.reads30, self.h1, self.h2, self.plain1, self.big1, self.big2, self.long1, self.short2):
            h.free()
        for b in self._buffers + [self.swap]:
            b.free()
        self._texts.clear()


# ================================================================ entries
class Entry:
    """One call.  run(sassy, searcher, fx) and expect(fx) return the same canonical value.
    kinds: ids of the kinds it applies to.  methods: the Searcher methods it names (tests/test_call_catalogue_cpu.py).
    route: {stats field: value} the call alone on a fresh searcher must show (None: nothing asserted), or a function of the
    kind.  big / small: a big sibling names its small one.  plain: a mode entry names the plain entry it must differ from.
    twin: the "same length, other bytes" entry names the entry it must differ from.  results: run_results(sassy, searcher, fx)
    -> the call's Result objects, for the walks that keep results alive; run() is then their canonical form.
    min_size: what expect() must hold at least (matches, records, merged pairs), counted by size_of."""

    def __init__(self, name, family, kinds, methods, run=None, expect=None, route=None, big=False, small=None, plain=None, twin=None,
                 results=None, size_of=None, refusal=False):
        self.name, self.family, self.kinds, self.methods = name, family, tuple(kinds), tuple(methods)
        self.results = results
        self._run = run
        self.expect, self._route, self.big, self.small, self.plain, self.twin = expect, route, big, small, plain, twin
        self.size_of = size_of or (lambda v: len(v))
        self.refusal = refusal

    def run(self, sassy, s, fx):
        if self.results is not None:
            return canon_results(sassy, self.results(sassy, s, fx))
        return self._run(sassy, s, fx)

    def route(self, kind):
        return self._route(kind) if callable(self._route) else self._route

    def __repr__(self):
        return "Entry(%s)" % self.name


ENTRIES = []


def entry(*a, **kw):
    e = Entry(*a, **kw)
    assert e.name not in {x.name for x in ENTRIES}, e.name
    ENTRIES.append(e)
    return e


def entries_for(kind):
    kid = kind.id if isinstance(kind, Kind) else kind
    return [e for e in ENTRIES if kid in e.kinds]


def by_name(name):
    return next(e for e in ENTRIES if e.name == name)


def _rows_size(v):
    """how many records a canonical matches value holds"""
    return v[1] if v and v[0] == "rows" else len(v)


# ---------------------------------------------------------------- single text
def _count_route(kind):
    # scan_route.h: m = 300 at k = 10 is eleven pieces -- more than the bit-plane filter's eight -- and the q-gram counting
    # filter (Q = 6: threshold 235 of 295 q-grams) is as selective as a filter gets.  One strand only: a searcher with rc marks
    # both strands in one pass of another kind, an Ascii searcher has no counting filter, an overhang searcher no filter at all.
    return {"filtered": 4} if kind.id in ("dna", "iupac") else {"filtered": 0} if kind.id == "iupac-alpha" else None


def _single(name, method, pattern, text, k, all_minima=False, without_trace=False, kinds=ALL, route=None, **kw):
    def run(sassy, s, fx):
        return canon_matches(getattr(s, method)(pattern(fx), text(fx), k))

    def expect(fx):
        recs = [rec(m) for m in fx.search(pattern(fx), text(fx), k, all_minima=all_minima)]
        if without_trace:
            recs = [bref.without_trace(r) for r in recs]
        return canon_records(recs)
    return entry(name, "scan", kinds, [method], run, expect, route=route, size_of=_rows_size, **kw)


_single("search", "search", lambda fx: fx.d.p20, lambda fx: fx.t1, 2)
_single("search_all", "search_all", lambda fx: fx.d.p20, lambda fx: fx.t1, 2, all_minima=True)
_single("search_without_trace", "search_without_trace", lambda fx: fx.d.p20, lambda fx: fx.t1, 2, without_trace=True)
_single("search_same_length_other_bytes", "search", lambda fx: fx.d.p20b, lambda fx: fx.t1, 2, twin="search")
_single("search_other_k", "search", lambda fx: fx.d.p20, lambda fx: fx.t1, 3)
_single("search_m300_k10", "search", lambda fx: fx.d.p300, lambda fx: fx.t1, 10, route=_count_route)
# five-row pieces: no filter applies, the streaming DP runs over every block
_single("search_streaming", "search", lambda fx: fx.d.p15, lambda fx: fx.t1, 2, route={"filtered": 0})
_single("search_low_complexity", "search", lambda fx: fx.d.p20, lambda fx: fx.d.t2, 2, kinds=PLAIN)
_single("search_all_microsatellite", "search_all", lambda fx: fx.d.pmicro, lambda fx: fx.d.t2, 2, all_minima=True, kinds=NUC)
_single("search_with_N", "search", lambda fx: fx.d.p20, lambda fx: fx.tn, 2, kinds=WITH_N)
_single("search_overhang_text", "search", lambda fx: fx.d.p20, lambda fx: fx.d.tov, 4, kinds=("iupac-alpha",))
_single("search_all_overhang_text", "search_all", lambda fx: fx.d.p20, lambda fx: fx.d.tov, 4, all_minima=True, kinds=("iupac-alpha",))
# the big sibling of search_all: more reports than the initial d_cand (65 536) and than kRankLimit (32 768).  It goes through
# Searcher._search -- what search_all wraps -- for the Result: 70 000 Match objects per call would cost the pair matrix,
# where the entry is a B to every A, more time than the rest of it takes
entry("search_all_poly_a_70000", "scan", PLAIN, ["search_all"],
      results=lambda sassy, s, fx: [s._search(fx.d.big_pat, fx.d.big_text, 2, sassy.ALL_MINIMA)],
      expect=lambda fx: (canon_matches(fx.search(fx.d.big_pat, fx.d.big_text, 2, all_minima=True), 0),),
      big=True, small="search_all", size_of=lambda v: _rows_size(v[0]))


def _with_fn_filter(pattern, text_till_end, strand):
    return len(text_till_end) % 2 == 0 or strand == "-"


entry("search_with_fn", "scan", PLAIN, ["search_with_fn"],
      lambda sassy, s, fx: canon_matches(s.search_with_fn(fx.d.p20, fx.t1, 2, True, _with_fn_filter)),
      lambda fx: canon_matches(fx.search(fx.d.p20, fx.t1, 2, all_minima=True, end_filter=_with_fn_filter), 0), size_of=_rows_size)

# class patterns (ascii kinds): P20 with rows 4, 10 and 16 opened to the class [XY]; T1 carries X and Y at those rows of two
# plants.  X and Y occur in no other row, so the class search is the oracle's search of the base pattern (X at the three
# rows) on the text with the class mapped onto its first member -- the construction of tests/test_gpu_classes.py
# (trace_shapes.mapped); an ascii_ci searcher closes the class under the case twin first.
CLASS_EXPR = b"ACGT[XY]GCAAG[XY]TCAGG[XY]CAT"
CLASS_BASE = b"ACGTXGCAAGXTCAGGXCAT"


def _class_run(sassy, s, fx):
    return canon_matches(s.search_classes(CLASS_EXPR, fx.d.t1_class, 2))


def _class_expected(fx):
    group = b"XYxy" if fx.profile == "ascii_ci" else b"XY"
    return canon_matches(fx.search(CLASS_BASE, mapped(fx.d.t1_class, [group]), 2), 0)


entry("search_classes", "scan", TEXTY, ["search_classes"], _class_run, _class_expected, route={"filtered": 0}, size_of=_rows_size)


def _lines_run(sassy, s, fx):
    matches, spans = s.search_lines(fx.d.p20, fx.tl, 2)
    return (canon_matches(matches), canon_struct(spans, SPAN_FIELDS))


def _lines_expect(fx):
    want = fx.search(fx.d.p20, fx.tl, 2)
    spans = np.array([lref.match_span(fx.tl, m.text_start, m.text_end) for m in want], dtype=[(f, dt) for f, dt in SPAN_FIELDS])
    return (canon_matches(want, 0), canon_struct(spans, SPAN_FIELDS))


entry("search_lines", "lines", PLAIN, ["search_lines"], _lines_run, _lines_expect, size_of=lambda v: len(v[0]))
SPAN_FIRST = [0, 78, 79, 80, 200, 3000, 6143, 6144]
SPAN_LAST = [0, 79, 79, 400, 219, 3000, 6143, 6144]
entry("line_spans", "lines", PLAIN, ["line_spans"],
      lambda sassy, s, fx: canon_struct(s.line_spans(fx.tl, SPAN_FIRST, SPAN_LAST), SPAN_FIELDS),
      lambda fx: canon_struct(np.array(lref.line_spans(fx.tl, SPAN_FIRST, SPAN_LAST), dtype=[(f, dt) for f, dt in SPAN_FIELDS]), SPAN_FIELDS),
      size_of=lambda v: v[0][2][0])


def _all_alignments_run(sassy, s, fx):
    return tuple(tuple(g) for g in aref.as_tuples(s.search_all_alignments(fx.d.p12, fx.t1, 1)))


entry("search_all_alignments", "scan", NUC, ["search_all_alignments"], _all_alignments_run,
      lambda fx: tuple(tuple(g) for g in aref.search_all_alignments(fx.profile, fx.d.p12, fx.t1, 1, rc=fx.rc)))


# --- a text that is resident on the device
def _dev_search(sassy, s, fx):
    return canon_matches(s.search(fx.d.p20, fx.dev.resident(fx.t1), 2))


entry("search_device_text", "scan", PLAIN, ["search"], _dev_search, lambda fx: canon_matches(fx.search(fx.d.p20, fx.t1, 2), 0), size_of=_rows_size)


def _dev_unchanged(sassy, s, fx):
    text = fx.dev.resident(fx.t1)
    first = s.search(fx.d.p20, text, 2)
    s.text_unchanged(True)
    try:
        second = s.search(fx.d.p20b, text, 2)
    finally:
        s.text_unchanged(False)
    return (canon_matches(first), canon_matches(second))


entry("search_device_text_unchanged", "scan", PLAIN, ["search", "text_unchanged"], _dev_unchanged,
      lambda fx: (canon_matches(fx.search(fx.d.p20, fx.t1, 2), 0), canon_matches(fx.search(fx.d.p20b, fx.t1, 2), 0)), size_of=lambda v: len(v[0]))


def _dev_rewritten(sassy, s, fx):
    """the same device pointer, new contents uploaded, flag off: nothing kept under the pointer may be used"""
    text = sassy.DeviceText(fx.dev.swap.ptr, len(fx.d.t1), owner=fx.dev.swap)
    out = []
    for contents in (fx.d.t1_swapped, fx.d.t1):
        fx.dev.swap.upload(contents)
        out.append(canon_matches(s.search(fx.d.p20, text, 2)))
    return tuple(out)


entry("search_device_text_rewritten", "scan", PLAIN, ["search"], _dev_rewritten,
      lambda fx: (canon_matches(fx.search(fx.d.p20, fx.d.t1_swapped, 2), 0), canon_matches(fx.search(fx.d.p20, fx.d.t1, 2), 0)),
      size_of=lambda v: len(v[0]))


# ---------------------------------------------------------------- reporting modes: set, call, restore
def _mode_only_best(sassy, s, fx):
    s.only_best_match(True)
    try:
        return canon_matches(s.search(fx.d.p20, fx.t1, 2))
    finally:
        s.only_best_match(False)


entry("mode_only_best_match", "modes", PLAIN, ["only_best_match", "search"], _mode_only_best,
      lambda fx: canon_matches(fx.search(fx.d.p20, fx.t1, 2, only_best=True), 0), plain="search")


def _mode_n_frac(sassy, s, fx):
    s.with_max_n_frac(0.05)
    try:
        return canon_matches(s.search(fx.d.p20, fx.tn, 2))
    finally:
        s.with_max_n_frac(None)


entry("mode_max_n_frac", "modes", WITH_N, ["with_max_n_frac", "search"], _mode_n_frac,
      lambda fx: canon_matches(fx.search(fx.d.p20, fx.tn, 2, max_n_frac=0.05), 0), plain="search_with_N")


def _mode_overhang(sassy, s, fx):
    s.with_max_overhang(2)
    try:
        return canon_matches(s.search(fx.d.p20, fx.d.tov, 4))
    finally:
        s.with_max_overhang(None)


entry("mode_max_overhang", "modes", ("iupac-alpha",), ["with_max_overhang", "search"], _mode_overhang,
      lambda fx: canon_matches(fx.search(fx.d.p20, fx.d.tov, 4, max_overhang=2), 0), plain="search_overhang_text")


def _mode_only_best_overhang(sassy, s, fx):
    s.only_best_match(True)
    try:
        return canon_matches(s.search(fx.d.p20, fx.d.tov, 4))
    finally:
        s.only_best_match(False)


entry("mode_only_best_match_overhang", "modes", ("iupac-alpha",), ["only_best_match", "search"], _mode_only_best_overhang,
      lambda fx: canon_matches(fx.search(fx.d.p20, fx.d.tov, 4, only_best=True), 0), plain="search_overhang_text")


# ---------------------------------------------------------------- many patterns or many texts
def _many_expected(fx, patterns, texts, k):
    pm = fx.pair_matches(patterns, texts, k)
    return canon_records([bref.record(m, ti, pi) for (pi, ti), ms in pm.items() for m in ms])


def _min_costs_expected(fx, patterns, texts, k):
    pm = fx.pair_matches(patterns, texts, k)
    cost = np.full((len(patterns), len(texts)), 255, dtype=np.uint8)
    strand = np.zeros((len(patterns), len(texts)), dtype=np.uint8)
    for (pi, ti), ms in pm.items():
        if ms:
            c, st = min((m.cost, bref.is_rc(m)) for m in ms)
            cost[pi, ti], strand[pi, ti] = c, st
    return canon_arrays((cost, strand))


def _best_pattern_expected(fx, patterns, texts, k):
    pm = fx.pair_matches(patterns, texts, k)
    cost, pattern, strand = np.full(len(texts), 255, dtype=np.uint8), np.full(len(texts), 0xFFFFFFFF, dtype=np.uint32), np.zeros(len(texts), np.uint8)
    for ti in range(len(texts)):
        cands = [(m.cost, pi, bref.is_rc(m)) for pi in range(len(patterns)) for m in pm[(pi, ti)]]
        if cands:
            cost[ti], pattern[ti], strand[ti] = min(cands)
    return canon_arrays((cost, pattern, strand))


def _best_matches_expected(fx, patterns, texts, k):
    pm = fx.pair_matches(patterns, texts, k)
    look = {(id(patterns[pi]), id(texts[ti])): ms for (pi, ti), ms in pm.items()}
    return canon_records(bref.expected(lambda p, t: look[(id(p), id(t))], patterns, texts))


def _reads(fx):
    return fx.dev.reads30


for _src, _texts, _kinds in (("list", lambda fx: fx.texts30, ALL), ("reads", _reads, NUC)):
    entry("search_many_" + _src, "many", _kinds, ["search_many"],
          results=lambda sassy, s, fx, _t=_texts: [s.search_many(fx.d.pats4, _t(fx), 2, as_result=True)],
          expect=lambda fx: (_many_expected(fx, fx.d.pats4, fx.texts30, 2),), size_of=lambda v: _rows_size(v[0]))
    _k2 = PLAIN if _src == "list" else NUC
    entry("min_costs_" + _src, "many", _k2, ["min_costs"],
          lambda sassy, s, fx, _t=_texts: canon_arrays(s.min_costs(fx.d.pats4, _t(fx), 2, strands=True)),
          lambda fx: _min_costs_expected(fx, fx.d.pats4, fx.texts30, 2), size_of=lambda v: v[0][1][0] * v[0][1][1])
    entry("best_pattern_" + _src, "many", _k2, ["best_pattern"],
          lambda sassy, s, fx, _t=_texts: canon_arrays(s.best_pattern(fx.d.pats4, _t(fx), 2)),
          lambda fx: _best_pattern_expected(fx, fx.d.pats4, fx.texts30, 2), size_of=lambda v: v[0][1][0])
    entry("best_matches_" + _src, "many", _k2, ["best_matches"],
          results=lambda sassy, s, fx, _t=_texts: [s.best_matches(fx.d.pats4, _t(fx), 2, as_result=True)],
          expect=lambda fx: (_best_matches_expected(fx, fx.d.pats4, fx.texts30, 2),), size_of=lambda v: _rows_size(v[0]))

entry("search_patterns", "many", PLAIN, ["search_patterns"],
      lambda sassy, s, fx: canon_matches(s.search_patterns(fx.d.pats4, fx.t1, 2)),
      lambda fx: _many_expected(fx, fx.d.pats4, [fx.t1], 2), size_of=_rows_size)
entry("search_texts", "many", PLAIN, ["search_texts"],
      lambda sassy, s, fx: canon_matches(s.search_texts(fx.d.p20, fx.texts30, 2)),
      lambda fx: _many_expected(fx, [fx.d.p20], fx.texts30, 2), size_of=_rows_size)


def _encoded_expected(fx, patterns, text, k):
    """oracle.search_encoded over slices of the patterns on THREADS threads (the C call releases the GIL)"""
    step = max(1, (len(patterns) + THREADS - 1) // THREADS)
    slices = [(a, patterns[a:a + step]) for a in range(0, len(patterns), step)]

    def one(job):
        a, ps = job
        return [bref.record(m, 0, a + m.pattern_idx) for m in oracle.search_encoded(fx.oprofile, ps, text, k, rc=fx.rc)]
    with ThreadPoolExecutor(THREADS) as ex:
        return canon_records([r for part in ex.map(one, slices) for r in part])


entry("search_encoded_tiled", "many", NUC, ["encode_patterns", "search_encoded_patterns"],
      results=lambda sassy, s, fx: [s.search_encoded_patterns(s.encode_patterns(fx.d.pats8), fx.t1, 2, as_result=True)],
      expect=lambda fx: (_encoded_expected(fx, fx.d.pats8, fx.t1, 2),), route={"filtered": 5}, size_of=lambda v: _rows_size(v[0]))
# the seeded route, on the smallest input that takes it (the docstring); one kind: the expectation is 1.3e10 DP cells
entry("search_encoded_seeded", "many", ("dna",), ["encode_patterns", "search_encoded_patterns"],
      results=lambda sassy, s, fx: [s.search_encoded_patterns(s.encode_patterns(fx.d.seeded_pats), fx.d.seeded_text, 2, as_result=True)],
      expect=lambda fx: (_encoded_expected(fx, fx.d.seeded_pats, fx.d.seeded_text, 2),), route={"filtered": 6},
      size_of=lambda v: _rows_size(v[0]))


# ---------------------------------------------------------------- Hamming
def _ham_one(fx, on_device):
    return fx.dev.resident(fx.t1) if on_device else fx.t1


def _ham_records(rows):
    return canon_records([(t,) + href.key(x) for t, x in rows])


HAM = {"filtered": 7}
for _src, _dev in (("host", False), ("device", True)):
    entry("search_hamming_" + _src, "hamming", PLAIN, ["search_hamming"],
          results=lambda sassy, s, fx, _d=_dev: [s.search_hamming(fx.d.hpats, _ham_one(fx, _d), 2, as_result=True)],
          expect=lambda fx: (_ham_records([(0, x) for x in href.expected(fx.profile, fx.d.hpats, fx.t1, 2, rc=fx.rc)]),), route=HAM,
          size_of=lambda v: _rows_size(v[0]))
    entry("hamming_counts_" + _src, "hamming", PLAIN, ["hamming_counts"],
          lambda sassy, s, fx, _d=_dev: canon_array(s.hamming_counts(fx.d.hpats, _ham_one(fx, _d), 2)),
          lambda fx: canon_array(hcref.expected_counts(fx.profile, fx.d.hpats, fx.t1, 2, rc=fx.rc)), route=HAM,
          size_of=lambda v: int(np.frombuffer(v[2], dtype=np.uint64).sum()))
    entry("hamming_amplicons_" + _src, "hamming", NUC, ["hamming_amplicons"],
          lambda sassy, s, fx, _d=_dev: canon_struct(s.hamming_amplicons(fx.d.primers, _ham_one(fx, _d), 1, 50, 1000), AMPLICON_FIELDS),
          lambda fx: canon_struct(amplicon_ref.expected(fx.profile, fx.d.primers, fx.t1, 1, 50, 1000, fx.rc), AMPLICON_FIELDS),
          size_of=lambda v: v[0][2][0])
for _src, _texts, _kinds in (("list", lambda fx: fx.texts30, PLAIN), ("reads", _reads, NUC)):
    entry("search_hamming_many_" + _src, "hamming", _kinds, ["search_hamming_many"],
          results=lambda sassy, s, fx, _t=_texts: [s.search_hamming_many(fx.d.hpats, _t(fx), 2, as_result=True)],
          expect=lambda fx: (_ham_records(hmref.expected_many(fx.profile, fx.d.hpats, fx.texts30, 2, rc=fx.rc)),), route=HAM,
          size_of=lambda v: _rows_size(v[0]))
    entry("hamming_best_pattern_" + _src, "hamming", _kinds, ["hamming_best_pattern"],
          lambda sassy, s, fx, _t=_texts: tuple(zip(*(a.tolist() for a in s.hamming_best_pattern(fx.d.hpats, _t(fx), 2)))),
          lambda fx: tuple(hmref.expected_best(fx.profile, fx.d.hpats, fx.texts30, 2, rc=fx.rc)), route=HAM)
    entry("hamming_counts_many_" + _src, "hamming", _kinds, ["hamming_counts_many"],
          lambda sassy, s, fx, _t=_texts: canon_array(s.hamming_counts_many(fx.d.hpats, _t(fx), 2)),
          lambda fx: canon_array(hcref.expected_counts(fx.profile, fx.d.hpats, list(fx.texts30), 2, rc=fx.rc)), route=HAM,
          size_of=lambda v: int(np.frombuffer(v[2], dtype=np.uint64).sum()))
# the big sibling: 20 000 hits
entry("search_hamming_20000_hits", "hamming", PLAIN, ["search_hamming"],
      results=lambda sassy, s, fx: [s.search_hamming(fx.d.big_ham_pat, fx.d.big_ham_text, 0, as_result=True)],
      expect=lambda fx: (_ham_records([(0, x) for x in href.expected(fx.profile, fx.d.big_ham_pat, fx.d.big_ham_text, 0, rc=fx.rc)]),),
      route=HAM, big=True, small="search_hamming_host", size_of=lambda v: _rows_size(v[0]))


# ---------------------------------------------------------------- sets
def _nearest(arrays):
    return canon_arrays([np.asarray(a).astype(dt) for a, dt in zip(arrays, (np.uint8, np.uint32, np.uint8, np.uint32))])


entry("hamming_pairs", "sets", PLAIN, ["hamming_pairs"],
      lambda sassy, s, fx: canon_struct(s.hamming_pairs(fx.d.set_a, None, 2), PAIR_FIELDS),
      lambda fx: canon_struct(pref.expected_pairs(fx.profile, fx.d.set_a, None, 2, rc=fx.rc), PAIR_FIELDS), route={"filtered": 8},
      size_of=lambda v: v[0][2][0])
entry("hamming_nearest", "sets", PLAIN, ["hamming_nearest"],
      lambda sassy, s, fx: _nearest(s.hamming_nearest(fx.d.set_a, fx.d.set_b, 3)),
      lambda fx: _nearest(pref.expected_nearest(fx.profile, fx.d.set_a, fx.d.set_b, 3, rc=fx.rc)), route={"filtered": 8}, size_of=lambda v: v[0][1][0])
entry("edit_pairs", "sets", PLAIN, ["edit_pairs"],
      lambda sassy, s, fx: canon_struct(s.edit_pairs(fx.d.set_a, None, 2), PAIR_FIELDS),
      lambda fx: canon_struct(eref.expected_pairs(fx.profile, fx.d.set_a, None, 2, rc=fx.rc), PAIR_FIELDS), route={"filtered": 9},
      size_of=lambda v: v[0][2][0])
entry("edit_nearest", "sets", PLAIN, ["edit_nearest"],
      lambda sassy, s, fx: _nearest(s.edit_nearest(fx.d.set_a, fx.d.set_b, 3)),
      lambda fx: _nearest(eref.expected_nearest(fx.profile, fx.d.set_a, fx.d.set_b, 3, rc=fx.rc)), route={"filtered": 9}, size_of=lambda v: v[0][1][0])


def _labels(arrays):
    return canon_arrays([np.asarray(a).astype(np.uint32) for a in arrays])


entry("hamming_clusters", "sets", PLAIN, ["hamming_clusters"],
      lambda sassy, s, fx: _labels(s.hamming_clusters(fx.d.set_a, 1)),
      lambda fx: _labels(clusters_ref.expected_clusters(fx.profile, fx.d.set_a, 1, rc=fx.rc)), route={"filtered": 10}, size_of=lambda v: v[0][1][0])
entry("edit_clusters", "sets", PLAIN, ["edit_clusters"],
      lambda sassy, s, fx: _labels(s.edit_clusters(fx.d.set_a, 1)),
      lambda fx: _labels(clusters_ref.expected_clusters(fx.profile, fx.d.set_a, 1, rc=fx.rc, edit=True)), route={"filtered": 11},
      size_of=lambda v: v[0][1][0])
for _method in uref.METHODS:
    entry("umi_groups_" + _method, "umi", PLAIN, ["umi_groups"],
          lambda sassy, s, fx, _m=_method: _labels(s.umi_groups(fx.d.umis, 1, _m)),
          lambda fx, _m=_method: _labels(uref.expected_umi_groups(fx.profile, fx.d.umis, 1, _m, rc=fx.rc)), route={"filtered": 12},
          size_of=lambda v: v[0][1][0])
# the big siblings: n = 3 000
entry("hamming_pairs_3000", "sets", PLAIN, ["hamming_pairs"],
      lambda sassy, s, fx: canon_struct(s.hamming_pairs(fx.d.set_big, None, 1), PAIR_FIELDS),
      lambda fx: canon_struct(pref.expected_pairs(fx.profile, fx.d.set_big, None, 1, rc=fx.rc), PAIR_FIELDS), route={"filtered": 8},
      big=True, small="hamming_pairs", size_of=lambda v: v[0][2][0])
entry("umi_groups_3000", "umi", PLAIN, ["umi_groups"],
      lambda sassy, s, fx: _labels(s.umi_groups(fx.d.set_big, 1, "directional")),
      lambda fx: _labels(uref.expected_umi_groups(fx.profile, fx.d.set_big, 1, "directional", rc=fx.rc)), route={"filtered": 12},
      big=True, small="umi_groups_directional", size_of=lambda v: v[0][1][0])


# ---------------------------------------------------------------- reads
def _parse_run(keep):
    def run(sassy, s, fx):
        h = sassy.DeviceReads(fx.d.fastq, keep_quality=keep)
        try:
            cols = tuple(canon_array(np.asarray(c).astype(np.uint64)) for c in (h.id_starts, h.id_lens, h.seq_starts, h.seq_lens, h.qual_starts,
                                                                               h.qual_lens))
            out = cols + (bytes(h.download_text()), canon_array(h.download_rem()), bool(h.qual_ptr),
                          bytes(h.download_quality_text()) if keep else None,
                          canon_array(s.hamming_counts_many(fx.d.hpats, h, 2)))   # ... and the searcher scans the new handle
        finally:
            h.free()
        return out
    return run


def _parse_expect(keep):
    def expect(fx):
        cols, src = fastq_ref.columns(fx.d.fastq)
        seqs = [sq for _, sq, _ in fastq_ref.records(fx.d.fastq)]
        return tuple(canon_array(cols[c].astype(np.uint64)) for c in ("id_start", "id_len", "seq_start", "seq_len", "qual_start", "qual_len")) + \
            (fastq_ref.layout_np(fx.d.fastq, cols, src).tobytes(), canon_array(fastq_ref.rem(cols["seq_start"], cols["seq_len"])), keep,
             mref.quality_layout(fx.d.fastq).tobytes() if keep else None,
             canon_array(hcref.expected_counts(fx.profile, fx.d.hpats, seqs, 2, rc=fx.rc)))
    return expect


entry("device_reads", "reads", NUC, ["hamming_counts_many"], _parse_run(False), _parse_expect(False), size_of=lambda v: v[0][1][0])
entry("device_reads_keep_quality", "reads", NUC, ["hamming_counts_many"], _parse_run(True), _parse_expect(True), size_of=lambda v: v[0][1][0])


def _fasta_run(sassy, s, fx):
    fa = sassy.DeviceFasta(fx.d.fasta)
    try:
        table = tuple(canon_array(np.asarray(c).astype(np.uint64)) for c in (fa.id_starts, fa.id_lens, fa.seq_starts, fa.seq_lens))
        return table + (canon_matches(s.search(fx.d.p20, fa.text(1), 2)),)
    finally:
        fa.free()


def _fasta_expect(fx):
    recs = fasta_ref.parse(fx.d.fasta)
    table = tuple(canon_array(np.array(c, dtype=np.uint64)) for c in ([r.id_start for r in recs], [r.id_len for r in recs],
                                                                        [r.seq_start for r in recs], [r.seq_len for r in recs]))
    return table + (canon_matches(fx.search(fx.d.p20, recs[1].seq, 2), 0),)


entry("device_fasta_search", "reads", NUC, ["search"], _fasta_run, _fasta_expect, size_of=lambda v: len(v[4]))

def _overlaps_expected(fx, r1s, r2s):
    key = ("overlaps", id(r1s))
    return fx.memo(key, lambda: oref.expected_overlaps(fx.profile, r1s, r2s, *fx.d.pair_call))


entry("read_overlaps", "overlaps", NUC, ["read_overlaps"],
      lambda sassy, s, fx: canon_struct(s.read_overlaps(fx.dev.h1, fx.dev.h2, *fx.d.pair_call), OVERLAP_FIELDS),
      lambda fx: canon_struct(_overlaps_expected(fx, [x[0] for x in fx.d.pairs1], [x[0] for x in fx.d.pairs2]), OVERLAP_FIELDS),
      size_of=lambda v: int(np.count_nonzero(np.frombuffer(v[3][3], dtype="<u4"))))
entry("read_overlaps_1100_pairs", "overlaps", NUC, ["read_overlaps"],
      lambda sassy, s, fx: canon_struct(s.read_overlaps(fx.dev.big1, fx.dev.big2, *fx.d.pair_call), OVERLAP_FIELDS),
      lambda fx: canon_struct(oref.expected_overlaps(fx.profile, fx.d.big_r1, fx.d.big_r2, *fx.d.pair_call), OVERLAP_FIELDS),
      big=True, small="read_overlaps", size_of=lambda v: int(np.count_nonzero(np.frombuffer(v[3][3], dtype="<u4"))))


def _merge_expected(fx):
    return fx.memo("merge", lambda: mref.expected_merge(fx.profile, fx.d.pairs1, fx.d.pairs2, *fx.d.pair_call))


def _merge_run(sassy, s, fx):
    merged, records = s.merge_pairs(fx.dev.h1, fx.dev.h2, *fx.d.pair_call, with_overlaps=True)
    try:
        return (canon_struct(records, OVERLAP_FIELDS),) + canon_handle(merged)
    finally:
        merged.free()


def _merge_expect(fx):
    records, seqs, quals = _merge_expected(fx)
    return (canon_struct(records, OVERLAP_FIELDS),) + expected_handle(seqs, quals)


entry("merge_pairs", "overlaps", NUC, ["merge_pairs"], _merge_run, _merge_expect,
      size_of=lambda v: int(np.count_nonzero(np.frombuffer(v[3][2], dtype="<u8"))))


def _merge_scan_pats(fx):
    seqs = _merge_expected(KIND_FIXTURES("dna"))[1]
    return [seqs[0][5:17], seqs[3][:12], oref.revcomp("dna", seqs[4][-12:]), b"ACGTACGTACGT"]


def _merge_scan_run(sassy, s, fx):
    merged = s.merge_pairs(fx.dev.h1, fx.dev.h2, *fx.d.pair_call)
    try:
        return canon_matches(s.search_many(_merge_scan_pats(fx), merged, 2))
    finally:
        merged.free()


entry("merge_pairs_then_scan", "overlaps", NUC, ["merge_pairs", "search_many"], _merge_scan_run,
      lambda fx: _many_expected(fx, _merge_scan_pats(fx), _merge_expected(fx)[1], 2), size_of=_rows_size)


# ---------------------------------------------------------------- in flight
def _shard_results(sassy, s, fx):
    t = fx.dev.resident(fx.t1)
    return [s.search_shard(fx.d.p20, t.data_ptr(), 0, len(fx.t1), 0, len(fx.t1), 2)]


def _fwd(fx, pattern, text, k):
    """shards are forward searches without reporting modes, whatever the searcher's strands"""
    return canon_matches(fx.search(pattern, text, k, rc=False), 0)


entry("search_shard", "in_flight", PLAIN, ["search_shard"], results=_shard_results, expect=lambda fx: (_fwd(fx, fx.d.p20, fx.t1, 2),),
      size_of=lambda v: _rows_size(v[0]))


def _in_flight_results(sassy, s, fx):
    """two begins, then both finishes; a searcher at pipe depth 1 takes one search in flight: then begin, finish, begin, finish"""
    t = fx.dev.resident(fx.t1)
    n = len(fx.t1)
    first = s.search_shard_begin(fx.d.p20, t.data_ptr(), 0, n, 0, n, 2)
    try:
        second = s.search_shard_begin(fx.d.p20b, t.data_ptr(), 0, n, 0, n, 2)
    except sassy.SassyHipError as e:
        if "too many searches in flight" not in str(e):
            s.search_finish(first)
            raise
        r1 = s.search_finish(first)
        return [r1, s.search_finish(s.search_shard_begin(fx.d.p20b, t.data_ptr(), 0, n, 0, n, 2))]
    r1 = s.search_finish(first)
    return [r1, s.search_finish(second)]


entry("search_shard_begin_twice_then_finish", "in_flight", PLAIN, ["search_shard_begin", "search_finish"], results=_in_flight_results,
      expect=lambda fx: (_fwd(fx, fx.d.p20, fx.t1, 2), _fwd(fx, fx.d.p20b, fx.t1, 2)), size_of=lambda v: _rows_size(v[0]))


# ---------------------------------------------------------------- refusals: the message's key words; nothing may stay behind
def _refusal(name, family, kinds, methods, call, words):
    def run(sassy, s, fx):
        try:
            call(sassy, s, fx)
        except sassy.SassyHipError as e:
            return tuple(w for w in words if w in str(e))
        return ("not refused",)
    return entry(name, family, kinds, methods, run, lambda fx: tuple(words), refusal=True)


_refusal("refused_class_pattern_wrong_profile", "scan", NUC + ("iupac-alpha",), ["search_classes"],
         lambda sassy, s, fx: s.search_classes(CLASS_EXPR, fx.t1, 1), ("class patterns need an ascii or ascii_ci searcher",))
_refusal("refused_amplicons_wrong_profile", "hamming", TEXTY, ["hamming_amplicons"],
         lambda sassy, s, fx: s.hamming_amplicons(fx.d.primers, fx.t1, 1, 50, 1000), ("dna and iupac searchers only",))
_refusal("refused_hamming_overhang", "hamming", ("iupac-alpha",), ["search_hamming"],
         lambda sassy, s, fx: s.search_hamming(fx.d.p20, fx.t1, 1), ("does not take overhang",))
_refusal("refused_empty_pattern", "scan", ALL, ["search"], lambda sassy, s, fx: s.search(b"", fx.t1, 1), ("empty pattern",))
_refusal("refused_null_text", "in_flight", ALL, ["search_shard"],
         lambda sassy, s, fx: s.search_shard(fx.d.p20, 0, 0, 64, 0, 64, 2), ("null argument",))
_refusal("refused_hamming_1025_rows", "hamming", PLAIN, ["search_hamming"],
         lambda sassy, s, fx: s.search_hamming(b"A" * 1025, fx.t1, 1), ("at most 1024 rows", "pattern 0 has 1025"))
_refusal("refused_pairs_129_columns", "sets", PLAIN, ["hamming_pairs"],
         lambda sassy, s, fx: s.hamming_pairs(np.full((3, 129), 65, dtype=np.uint8), None, 1), ("m must be <= 128", "got 129"))
_refusal("refused_umi_129_columns", "umi", PLAIN, ["umi_groups"],
         lambda sassy, s, fx: s.umi_groups(np.full((3, 129), 65, dtype=np.uint8), 1), ("umi_groups", "m must be <= 128"))
_refusal("refused_min_costs_k_255", "many", ALL, ["min_costs"],
         lambda sassy, s, fx: s.min_costs(fx.d.pats4, fx.texts30, 255), ("k must be <= 254",))
_refusal("refused_line_span_backwards", "lines", ALL, ["line_spans"],
         lambda sassy, s, fx: s.line_spans(fx.tl, [5], [3]), ("span 0 is not first <= last <= text_len",))
_refusal("refused_overlaps_513_bytes", "overlaps", NUC, ["read_overlaps"],
         lambda sassy, s, fx: s.read_overlaps(fx.dev.long1, fx.dev.short2), ("at most 512 bytes",))
_refusal("refused_merge_without_qualities", "overlaps", NUC, ["merge_pairs"],
         lambda sassy, s, fx: s.merge_pairs(fx.dev.plain1, fx.dev.h2), ("KEEP_QUALITY",))


# ================================================================ one Fixtures per kind, and all expectations at once
_FIXTURES = {}


def KIND_FIXTURES(kind_id):
    if kind_id not in _FIXTURES:
        _FIXTURES[kind_id] = Fixtures(KIND[kind_id])
    return _FIXTURES[kind_id]


_EXPECTED = {}


def expected(kind_id, name):
    """expect() of one entry under one kind, computed once per process"""
    key = (kind_id, name)
    if key not in _EXPECTED:
        _EXPECTED[key] = by_name(name).expect(KIND_FIXTURES(kind_id))
    return _EXPECTED[key]


def build_all_expectations(threads=THREADS):
    """every (kind, entry) expectation, on `threads` threads (the oracle's C calls and numpy release the GIL)"""
    jobs = [(k.id, e.name) for k in KINDS for e in entries_for(k)]
    data()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda j: expected(*j), jobs))
    return len(jobs)
