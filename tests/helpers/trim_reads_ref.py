"""Adapter and quality trimming of a read batch (sassy_hip_trim_reads, Searcher.trim_reads) restated in numpy and plain Python.
The relation is hamming_ref.relation_row (read off the oracle's DP): this file holds no second copy of it.  All arithmetic is
integer; there are no floats.

Read a of la bytes with qualities q; adapters p_0 .. p_{A-1}, p_j of m_j bytes, 5'->3' as they appear behind the insert.

Quality trim (the BWA / cutadapt 3' rule, Phred+33): quality_cutoff == 0: lq = la.  Otherwise walk i = la - 1 .. 0 with
s += q[i] - 33 - quality_cutoff; stop at the first i where s > 0; lq is the i of the strictly smallest s seen before the stop
(s < min, min starting at 0), la where no s was below 0.

Adapter, on a[0:lq]: position c places p_j[0] under a[c]; ov = min(m_j, lq - c); mm(c, j) = #{ i < ov : !match(p_j[i], a[c + i]) }
with the adapter on the pattern side.  Accepted: ov >= min_overlap, mm <= k, mm * 1000 <= max_permille * ov.  Best: the smallest
c, then the lower density (mm1 * ov2 < mm2 * ov1), then the larger ov, then the smaller j.

cut = c of the best, or lq; length = cut if cut >= min_length else 0.  The record is (length, quality_len = lq, adapter_pos =
cut, adapter = j or -1, overlap, mismatches), the last two 0 where no adapter was found."""
import numpy as np

from hamming_ref import relation_row

DTYPE = np.dtype([("length", "<u4"), ("quality_len", "<u4"), ("adapter_pos", "<u4"), ("adapter", "<i2"), ("overlap", "u1"), ("mismatches", "u1")])
assert DTYPE.itemsize == 16

# the issue's cases by hand, dna; each names its own call
_AD = b"AGATCGGAAGAGC"
HAND = [
    # a whole adapter in the middle
    dict(name="whole adapter in the middle", seq=b"ACGTTGCAAC" + _AD + b"TTTTT", qual=b"I" * 28, adapters=[_AD],
         call=dict(min_overlap=3, k=512, max_permille=100, quality_cutoff=0, min_length=0), record=(10, 28, 10, 0, 13, 0)),
    # a 4-base prefix of the adapter at the read's end
    dict(name="4-base prefix at the end", seq=b"ACGTTGCAACCT" + _AD[:4], qual=b"I" * 16, adapters=[_AD],
         call=dict(min_overlap=3, k=512, max_permille=100, quality_cutoff=0, min_length=0), record=(12, 16, 12, 0, 4, 0)),
    # cutoff 20, '#' = Phred 2 (term -18), 'I' = Phred 40 (term +20): from the right -18 -18 (s = -36 at i = 10), then +20 +20
    # (s = +4 at i = 8: stop).  The eight '#' further left would take s down to -140 at i = 0 and win without the stop.  lq = 10.
    dict(name="the early stop of the quality walk", seq=b"ACGTACGTACGT", qual=b"########II##",
         adapters=[], call=dict(min_overlap=3, k=512, max_permille=100, quality_cutoff=20, min_length=0), record=(10, 10, 10, -1, 0, 0)),
    # two adapters accepted at one c, equal density and overlap: the smaller j
    dict(name="two adapters at one position", seq=b"ACGTTGCAAC" + _AD, qual=b"I" * 23, adapters=[b"TTTTTTTT", _AD, _AD, _AD[:8]],
         call=dict(min_overlap=3, k=512, max_permille=100, quality_cutoff=0, min_length=0), record=(10, 23, 10, 1, 13, 0)),
    # dropped by min_length: the cut is kept in adapter_pos
    dict(name="dropped by min_length", seq=b"ACGTT" + _AD, qual=b"I" * 18, adapters=[_AD],
         call=dict(min_overlap=3, k=512, max_permille=100, quality_cutoff=0, min_length=6), record=(0, 18, 5, 0, 13, 0)),
]


def quality_len(qual: bytes, quality_cutoff: int) -> int:
    """lq: vectorised -- the suffix sums, the first positive one from the right, the strictly smallest before it."""
    la = len(qual)
    if quality_cutoff == 0 or la == 0:
        return la
    terms = np.frombuffer(bytes(qual), dtype=np.uint8).astype(np.int64) - 33 - int(quality_cutoff)
    s = np.cumsum(terms[::-1])[::-1]             # s[i] = the walk's sum when it stands at i
    pos = np.flatnonzero(s > 0)
    stop = int(pos[-1]) if pos.size else -1      # the walk looks at i > stop only
    tail = s[stop + 1:]
    if tail.size == 0 or tail.min() >= 0:
        return la
    # the first i from the right that reaches the minimum: the largest index
    return stop + 1 + int(np.flatnonzero(tail == tail.min())[-1])


def positions_table(profile: str, seq: bytes, lq: int, adapter: bytes):
    """(c, ov, mm) of every position 0 <= c < lq of one adapter, as int64 arrays."""
    a = np.frombuffer(bytes(seq), dtype=np.uint8)[:lq]
    m = len(adapter)
    c = np.arange(lq, dtype=np.int64)
    ov = np.minimum(m, lq - c)
    if lq == 0:
        return c, ov, c.copy()
    mis = ~np.stack([relation_row(profile, int(p)) for p in adapter])[:, a]   # (m, lq): adapter row i against read byte t mismatches
    padded = np.zeros((m, lq + m), dtype=np.int64)
    padded[:, :lq] = mis
    mm = sum(padded[i, i:i + lq] for i in range(m))                            # rows behind lq count nothing
    return c, ov, mm


def trim_one(profile: str, seq: bytes, qual, adapters, min_overlap=3, k=512, max_permille=100, quality_cutoff=0, min_length=0):
    """The record of one read as a tuple in DTYPE's order."""
    la = len(seq)
    lq = quality_len(qual, quality_cutoff) if quality_cutoff else la
    best = None  # (c, mm, ov, j)
    for j, ad in enumerate(adapters):
        c, ov, mm = positions_table(profile, seq, lq, bytes(ad))
        ok = np.flatnonzero((ov >= min_overlap) & (mm <= k) & (mm * 1000 <= max_permille * ov))
        if not ok.size:
            continue
        i = int(ok[0])  # the smallest c of this adapter; the other levels compare across adapters
        cand = (int(c[i]), int(mm[i]), int(ov[i]), j)
        if best is None or cand[0] < best[0] or (cand[0] == best[0] and (
                cand[1] * best[2] < best[1] * cand[2] or (cand[1] * best[2] == best[1] * cand[2] and cand[2] > best[2]))):
            best = cand
    cut = best[0] if best else lq
    length = cut if cut >= min_length else 0
    return (length, lq, cut, best[3] if best else -1, best[2] if best else 0, best[1] if best else 0)


def expected_trim(profile: str, reads, adapters, min_overlap=3, k=512, max_permille=100, quality_cutoff=0, min_length=0):
    """reads: [(sequence, quality)] or [sequence] (then quality_cutoff must be 0 and the qualities come back None).  Returns
    (records, [trimmed sequence], [trimmed quality])."""
    records = np.zeros(len(reads), dtype=DTYPE)
    seqs, quals = [], []
    for r, item in enumerate(reads):
        s, q = (item if isinstance(item, tuple) else (item, None))
        s = s.encode() if isinstance(s, str) else bytes(s)
        assert q is not None or quality_cutoff == 0
        rec = trim_one(profile, s, q, adapters, min_overlap, k, max_permille, quality_cutoff, min_length)
        records[r] = rec
        seqs.append(s[:rec[0]])
        quals.append(None if q is None else bytes(q)[:rec[0]])
    return records, seqs, quals
