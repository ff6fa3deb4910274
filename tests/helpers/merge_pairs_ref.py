"""The paired-end merge (sassy_hip_merge_pairs, Searcher.merge_pairs) restated in numpy.  The overlap rule is
read_overlaps_ref's and the complement is the oracle's through read_overlaps_ref.revcomp: this file holds no second copy of
either.

Pair r: a = read r of R1 with qualities qa, b = reverse_complement(profile, read r of R2), qb = R2's qualities reversed,
(d, ov, mm, n_acc) = the pair's read_overlaps record.  n_acc == 0: not merged, the merged read is empty.  Otherwise
L = max(la, d + lb) for d >= 0 and L = ov for d < 0; column p is a[p] where p < la and b[p - d] where 0 <= p - d < lb.  One
read covers p: its byte and quality.  Both, equal bytes: that byte, max(qa, qb).  Both, different bytes (whatever the
profile's relation says): the byte of the higher quality, a's on a tie, quality min(126, 33 + max(2, |qa - qb|)).  No quality
byte is validated."""
import numpy as np

import fastq_ref
import read_overlaps_ref as oref

# the issue's three cases by hand: dna, min_overlap = 4, k = 1, max_permille = 200
HAND_CALL = dict(min_overlap=4, k=1, max_permille=200)
HAND = [
    dict(r1=b"AAACCCGGG", q1=b"IIIIIIIII", r2=b"AAACCCGGG", q2=b"#########", record=(3, 6, 0, 2), merged=b"AAACCCGGGTTT", quality=b"IIIIIIIII###"),
    # column 4: T at 10 against C at 40, so C with 33 + 30
    dict(r1=b"AAACTCGGG", q1=b"IIII+IIII", r2=b"AAACCCGGG", q2=b"#######I#", record=(3, 6, 1, 1), merged=b"AAACCCGGGTTT", quality=b"IIII?IIII###"),
    # read-through
    dict(r1=b"ACGTACGG", q1=b"IIIIIIII", r2=b"GTACGTTT", q2=b"55555555", record=(-2, 6, 0, 1), merged=b"ACGTAC", quality=b"IIIIII"),
]


def merged_length(rec, la: int, lb: int) -> int:
    d, ov, n = int(rec[0]), int(rec[1]), int(rec[3])
    if n == 0:
        return 0
    return max(la, d + lb) if d >= 0 else ov


def merge_one(profile: str, r1: bytes, q1: bytes, r2: bytes, q2: bytes, rec):
    """(merged sequence, merged quality) of one pair under its record."""
    a, qa = np.frombuffer(bytes(r1), dtype=np.uint8).astype(np.int64), np.frombuffer(bytes(q1), dtype=np.uint8).astype(np.int64)
    b = np.frombuffer(oref.revcomp(profile, bytes(r2)), dtype=np.uint8).astype(np.int64)
    qb = np.frombuffer(bytes(q2), dtype=np.uint8).astype(np.int64)[::-1]
    la, lb, d = len(a), len(b), int(rec[0])
    assert len(qa) == la and len(qb) == lb
    L = merged_length(rec, la, lb)
    if L == 0:
        return b"", b""
    p = np.arange(L)
    in_a, in_b = p < la, (p - d >= 0) & (p - d < lb)
    assert (in_a | in_b).all()
    ca, xa = a[np.minimum(p, la - 1)], qa[np.minimum(p, la - 1)]
    j = np.clip(p - d, 0, lb - 1)
    cb, xb = b[j], qb[j]
    both, equal, a_wins = in_a & in_b, ca == cb, xa >= xb
    c = np.where(both, np.where(a_wins, ca, cb), np.where(in_a, ca, cb))
    q_both = np.where(equal, np.maximum(xa, xb), np.minimum(126, 33 + np.maximum(2, np.abs(xa - xb))))
    q = np.where(both, q_both, np.where(in_a, xa, xb))
    return c.astype(np.uint8).tobytes(), q.astype(np.uint8).tobytes()


def expected_merge(profile: str, pairs1, pairs2, min_overlap: int = 10, k: int = 512, max_permille: int = 200):
    """pairs1 / pairs2: [(sequence, quality)] of R1 and of R2.  Returns (records, [merged sequence], [merged quality]): one
    entry per pair, empty where the pair is not merged."""
    records = oref.expected_overlaps(profile, [x[0] for x in pairs1], [x[0] for x in pairs2], min_overlap, k, max_permille)
    seqs, quals = [], []
    for (r1, q1), (r2, q2), rec in zip(pairs1, pairs2, records):
        s, q = merge_one(profile, r1, q1, r2, q2, tuple(rec.tolist()))
        seqs.append(s)
        quals.append(q)
    return records, seqs, quals


def layout_of(seqs):
    """(starts, lens, buffer) of a list of byte strings under the read batch's layout rule: every string from a multiple of 64
    on, an empty one takes no block, zero pads, 64 zero bytes behind the last.  The same rule lays out the qualities."""
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    slot = (lens + np.uint64(63)) // np.uint64(64) * np.uint64(64)
    starts = (np.cumsum(slot) - slot).astype(np.uint64) if len(seqs) else np.zeros(0, dtype=np.uint64)
    out = np.zeros(int(slot.sum()) + 64, dtype=np.uint8)
    for s, at in zip(seqs, starts.tolist()):
        out[at:at + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    return starts, lens, out


def quality_layout(raw: bytes) -> np.ndarray:
    """The quality buffer of a handle parsed with keep_quality out of `raw`: the qualities in the text's layout."""
    return layout_of([q for _, _, q in fastq_ref.records(raw)])[2]


def rem_of(starts, lens) -> np.ndarray:
    return fastq_ref.rem(starts, lens)
