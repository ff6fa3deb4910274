"""Demultiplexing of a read batch (sassy_hip_demux_reads, DeviceReads.demux) and the gather (sassy_hip_reads_select) restated in
numpy.  The relation is hamming_ref.relation_row (read off the oracle's DP): this file holds no second copy of it.  All
arithmetic is integer; there are no floats.

Read a of la bytes; barcodes p_0 .. p_{B-1}, all of ONE length m, on the pattern side (an Iupac N in a barcode is a wildcard).

Window: from the 5' end w = at, from the 3' end w = la - at - m; the read has a window iff at + m <= la.
cost_j = #{ i < m : !match(p_j[i], a[w + i]) }.  best = the smallest j of the minimum cost, cost = that minimum, n_best = the
number of j at that cost, second = the minimum over j != best, m + 1 when B == 1.
Assigned iff the read has a window, cost <= k and second - cost >= min_delta.  The label is best if assigned, else B.
order = the stable argsort of the labels; bounds[s], s = 0 .. B + 1, = the first place of label s.
Output record j is read order[j]: an assigned read under clipping keeps [at + m, la) (5') or [0, la - at - m) (3'); any other
read is kept whole.  The record of read r is (sample = best or -1, best, cost, second, n_best, index = the place of r in the
output); a read without a window has (-1, 2^32 - 1, 255, 255, 0, index)."""
import numpy as np

from hamming_ref import relation_row

DTYPE = np.dtype([("sample", "<i4"), ("best", "<u4"), ("cost", "u1"), ("second", "u1"), ("n_best", "<u2"), ("index", "<u4")])
assert DTYPE.itemsize == 16
NO_BEST = 0xFFFFFFFF

# cases by hand, dna, barcodes of 4; each names its own call and its (sample, best, cost, second, n_best) and what is kept
_BC = [b"ACGT", b"TTAA", b"GGCC"]
HAND = [
    # the first barcode exactly at the 5' end: the other two differ from it in all four rows
    dict(name="exact at the 5' end", seq=b"ACGTTTGCA", barcodes=_BC, call=dict(k=1, min_delta=1, at=0, end3=False, clip=True),
         record=(0, 0, 0, 4, 1), kept=b"TTGCA"),
    # one substitution (ACCT: cost 1 to ACGT, 4 to TTAA, 3 to GGCC whose third row matches), behind a two-base spacer that goes
    # with the barcode
    dict(name="one substitution behind a spacer", seq=b"GGACCTGATTACA", barcodes=_BC, call=dict(k=1, min_delta=1, at=2, end3=False, clip=True),
         record=(0, 0, 1, 3, 1), kept=b"GATTACA"),
    # ACAA against ACGT mismatches in rows 2, 3 (cost 2), against TTAA in rows 0, 1 (cost 2), against GGCC in all four: a tie
    dict(name="a tie is unassigned under min_delta 1", seq=b"ACAAGGGG", barcodes=_BC, call=dict(k=2, min_delta=1, at=0, end3=False, clip=True),
         record=(-1, 0, 2, 2, 2), kept=b"ACAAGGGG"),
    dict(name="a tie goes to the smaller index under min_delta 0", seq=b"ACAAGGGG", barcodes=_BC, call=dict(k=2, min_delta=0, at=0, end3=False, clip=True),
         record=(0, 0, 2, 2, 2), kept=b"GGGG"),
    # the barcode one base in front of the 3' end; the base behind it goes with it
    dict(name="from the 3' end", seq=b"CATCATTTAAG", barcodes=_BC, call=dict(k=0, min_delta=1, at=1, end3=True, clip=True),
         record=(1, 1, 0, 4, 1), kept=b"CATCAT"),
    # too short for a window
    dict(name="no window", seq=b"ACG", barcodes=_BC, call=dict(k=4, min_delta=0, at=0, end3=False, clip=True),
         record=(-1, NO_BEST, 255, 255, 0), kept=b"ACG"),
    # one barcode: second = m + 1, so any margin up to m + 1 - cost holds
    dict(name="a single barcode", seq=b"ACGAAA", barcodes=[b"ACGT"], call=dict(k=1, min_delta=4, at=0, end3=False, clip=False),
         record=(0, 0, 1, 5, 1), kept=b"ACGAAA"),
]


def costs_table(profile: str, reads, barcodes, at: int, end3: bool):
    """(has_window (n,) bool, costs (n, B) int64; rows without a window are zero)."""
    m, B, n = len(barcodes[0]), len(barcodes), len(reads)
    assert all(len(b) == m for b in barcodes) and 1 <= m <= 64
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    has = lens >= at + m
    win = np.zeros((n, m), dtype=np.uint8)
    for r in np.flatnonzero(has).tolist():
        w = len(reads[r]) - at - m if end3 else at
        win[r] = np.frombuffer(bytes(reads[r][w:w + m]), dtype=np.uint8)
    costs = np.zeros((n, B), dtype=np.int64)
    for j, bc in enumerate(barcodes):
        for i, p in enumerate(bytes(bc)):
            costs[:, j] += ~relation_row(profile, p)[win[:, i]]
    costs[~has] = 0
    return has, costs


def expected_demux(profile: str, reads, barcodes, k=1, min_delta=1, at=0, end3=False, clip=True):
    """reads: [sequence] or [(sequence, quality)].  Returns (records, order, bounds, [kept sequence], [kept quality or None]) --
    the last two in the OUTPUT's order."""
    seqs = [bytes(x[0] if isinstance(x, tuple) else x) for x in reads]
    quals = [bytes(x[1]) if isinstance(x, tuple) else None for x in reads]
    barcodes = [bytes(b) for b in barcodes]
    m, B, n = len(barcodes[0]), len(barcodes), len(seqs)
    has, costs = costs_table(profile, seqs, barcodes, at, end3)
    records = np.zeros(n, dtype=DTYPE)
    if n:
        best = np.argmin(costs, axis=1)                     # the first of the minima
        cost = costs[np.arange(n), best]
        n_best = (costs == cost[:, None]).sum(axis=1)
        others = costs.copy()
        others[np.arange(n), best] = m + 1
        second = others.min(axis=1) if B > 1 else np.full(n, m + 1, dtype=np.int64)
        assigned = has & (cost <= k) & (second - cost >= min_delta)
        records["sample"] = np.where(assigned, best, -1)
        records["best"] = np.where(has, best, NO_BEST)
        records["cost"] = np.where(has, cost, 255)
        records["second"] = np.where(has, second, 255)
        records["n_best"] = np.where(has, n_best, 0)
        labels = np.where(assigned, best, B)
    else:
        assigned, labels = np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int64)
    order = np.argsort(labels, kind="stable").astype(np.uint64)
    records["index"][order.astype(np.int64)] = np.arange(n, dtype=np.uint32)
    bounds = np.searchsorted(labels[order.astype(np.int64)], np.arange(B + 2), side="left").astype(np.uint64)
    out_s, out_q = [], []
    for r in order.tolist():
        la = len(seqs[r])
        lo, hi = 0, la
        if assigned[r] and clip:
            lo, hi = (0, la - at - m) if end3 else (at + m, la)
        out_s.append(seqs[r][lo:hi])
        out_q.append(None if quals[r] is None else quals[r][lo:hi])
    return records, order, bounds, out_s, out_q


def expected_select(reads, src, begins=None, lens=None):
    """[(sequence, quality or None)] of the gather: record j = window j of read src[j]; begins, lens: per record, or one number."""
    out = []
    if begins is not None:
        begins, lens = np.broadcast_to(np.asarray(begins), (len(src),)), np.broadcast_to(np.asarray(lens), (len(src),))
    for j, r in enumerate(src):
        s, q = reads[r] if isinstance(reads[r], tuple) else (reads[r], None)
        lo = 0 if begins is None else int(begins[j])
        hi = len(s) if lens is None else lo + int(lens[j])
        assert 0 <= lo <= hi <= len(s)
        out.append((bytes(s[lo:hi]), None if q is None else bytes(q[lo:hi])))
    return out


def layout(seqs, quals=None):
    """The device buffers of a handle that holds these reads: (text, quality or None, starts, rem, longest) -- every read at the
    next multiple of 64, zeros behind it, 64 spare bytes behind the layout."""
    starts, at = [], 0
    for s in seqs:
        starts.append(at)
        at += (len(s) + 63) // 64 * 64
    text = np.zeros(at + 64, dtype=np.uint8)
    qual = np.zeros(at + 64, dtype=np.uint8) if quals is not None else None
    rem = np.zeros(at // 64, dtype=np.uint32)
    for i, s in enumerate(seqs):
        text[starts[i]:starts[i] + len(s)] = np.frombuffer(s, dtype=np.uint8)
        if quals is not None:
            qual[starts[i]:starts[i] + len(s)] = np.frombuffer(quals[i], dtype=np.uint8)
        for b in range((len(s) + 63) // 64):
            rem[starts[i] // 64 + b] = len(s) - 64 * b
    return text.tobytes(), None if qual is None else qual.tobytes(), np.array(starts, dtype=np.uint64), rem, max([len(s) for s in seqs], default=0)


def mixed_batch(n: int, seed: int, barcodes, at: int = 0, end3: bool = False, with_quality: bool = True, letters: bytes = b"ACGT"):
    """A seeded batch for k = 1, min_delta = 1 whose five groups each hold about a fifth of the reads: assigned at cost 0,
    assigned at cost 1, unassigned by k (three substitutions), unassigned by the margin (the window is one substitution from
    two barcodes -- the first two barcodes must be at distance 2 --), no window (too short, empty ones among them)."""
    rnd = np.random.RandomState(seed)
    m = len(barcodes[0])
    pick = lambda k_: bytes(rnd.choice(np.frombuffer(letters, dtype=np.uint8), size=k_).tolist())
    other = lambda c: bytes([letters[(letters.index(c) + 1 + rnd.randint(len(letters) - 1)) % len(letters)]])
    reads = []
    for r in range(n):
        kind = r % 5 if n >= 5 else rnd.randint(5)
        bc = bytearray(barcodes[rnd.randint(len(barcodes))])
        if kind == 1:
            i = rnd.randint(m)
            bc[i:i + 1] = other(bc[i])
        elif kind == 2:
            for i in rnd.choice(m, size=min(3, m), replace=False).tolist():
                bc[i:i + 1] = other(bc[i])
        elif kind == 3:  # between barcode 0 and barcode 1: one row from each
            a, b = barcodes[0], barcodes[1]
            diff = [i for i in range(m) if a[i] != b[i]]
            bc = bytearray(a)
            bc[diff[0]] = b[diff[0]]
        if kind == 4:
            la = rnd.randint(0, at + m) if rnd.randint(3) else 0
            seq = pick(la)
        else:
            head, tail = pick(at), pick(rnd.randint(0, 90))
            seq = (tail + bytes(bc) + head) if end3 else (head + bytes(bc) + tail)
        reads.append((seq, bytes(rnd.randint(33, 74, size=len(seq)).astype(np.uint8).tolist())) if with_quality else seq)
    return reads


def groups(records, k: int):
    """How many reads fall into each of the five groups the mixed batch must hold."""
    has = records["n_best"] > 0
    a = records["sample"] >= 0
    return dict(cost0=int((a & (records["cost"] == 0)).sum()), cost1=int((a & (records["cost"] >= 1)).sum()),
                by_k=int((has & ~a & (records["cost"] > k)).sum()), by_margin=int((has & ~a & (records["cost"] <= k)).sum()),
                no_window=int((~has).sum()))
