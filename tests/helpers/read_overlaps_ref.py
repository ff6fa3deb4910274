"""The paired-end overlap call (sassy_hip_read_overlaps) restated in numpy.  The relation is hamming_ref.relation_row (read off
the oracle's DP), the reverse complement is oracle.reverse_complement: this file holds no second copy of either.

Pair r: a = read r of R1, b = reverse_complement(profile, read r of R2).  The offset d, -(lb - 1) <= d <= la - 1, places b[0]
under a[d]; lo = max(0, d), hi = min(la, d + lb), ov = hi - lo, mm(d) = #{ i in [lo, hi) : !match(a[i], b[i - d]) } with a on
the pattern side.  Accepted: ov >= min_overlap, mm <= k, mm * 1000 <= max_permille * ov.  Best: the lower mm / ov
(cross-multiplied), then the larger ov, then the larger d.  The record is (d, ov, mm, n_accepted), all zero without an
accepted offset or with an empty read."""
import numpy as np

import oracle
from hamming_ref import relation_row

DTYPE = np.dtype([("offset", "<i4"), ("overlap", "<u4"), ("mismatches", "<u4"), ("n_accepted", "<u4")])

# the issue's two cases by hand: dna, k = 0, max_permille = 0
HAND = [
    dict(r1=b"AAACCCGGG", r2=b"AAACCCGGG", b=b"CCCGGGTTT", min_overlap=4, record=(3, 6, 0, 1), trims=(12, 9, 9)),
    dict(r1=b"ACGTACGG", r2=b"GTACGTTT", b=b"AAACGTAC", min_overlap=5, record=(-2, 6, 0, 1), trims=(6, 6, 6)),
]


def offsets_table(profile: str, r1: bytes, r2: bytes):
    """(d, ov, mm) of every offset of one pair as int64 arrays, d ascending; empty where a read is empty."""
    a = np.frombuffer(bytes(r1), dtype=np.uint8)
    b = np.frombuffer(oracle.reverse_complement(profile, bytes(r2)), dtype=np.uint8)
    la, lb = len(a), len(b)
    if la == 0 or lb == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    mis = ~np.stack([relation_row(profile, int(c)) for c in a])[:, b]  # (la, lb): a[i] against b[j] mismatches
    ds = np.arange(-(lb - 1), la, dtype=np.int64)
    mm = np.array([np.trace(mis, offset=-int(d)) for d in ds], dtype=np.int64)  # the diagonal i - j == d
    ov = np.minimum(la, ds + lb) - np.maximum(0, ds)
    return ds, ov, mm


def best_of(ds, ov, mm, min_overlap: int, k: int, max_permille: int):
    """The record of one pair out of its offsets' table."""
    ok = (ov >= min_overlap) & (mm <= k) & (mm * 1000 <= max_permille * ov)
    best = None
    for d, o, m in zip(ds[ok].tolist(), ov[ok].tolist(), mm[ok].tolist()):
        if best is None or m * best[1] < best[2] * o or (m * best[1] == best[2] * o and (o > best[1] or (o == best[1] and d > best[0]))):
            best = (d, o, m)
    return (best[0], best[1], best[2], int(ok.sum())) if best else (0, 0, 0, 0)


def expected_overlaps(profile: str, r1s, r2s, min_overlap: int = 10, k: int = 512, max_permille: int = 200) -> np.ndarray:
    assert len(r1s) == len(r2s)
    out = np.zeros(len(r1s), dtype=DTYPE)
    for r, (x, y) in enumerate(zip(r1s, r2s)):
        out[r] = best_of(*offsets_table(profile, x, y), min_overlap, k, max_permille)
    return out


def trims(rec, la: int, lb: int):
    """(insert, keep1, keep2) as the issue derives them from a record."""
    d, ov, n = int(rec[0]), int(rec[1]), int(rec[3])
    if n == 0:
        return 0, la, lb
    if d >= 0:
        return max(la, d + lb), la, lb
    return ov, min(la, d + lb), lb + d


def revcomp(profile: str, seq: bytes) -> bytes:
    return oracle.reverse_complement(profile, bytes(seq))


def planted_pair(rng, profile: str, la: int, lb: int, d: int, subs: int = 0, alphabet: bytes = b"ACGT"):
    """(r1, r2) whose b lies under a at offset d exactly but for `subs` substitutions inside the overlap; the rest random.
    Needs an overlap at d (or an empty read)."""
    a = bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), la).astype(np.uint8)) if la else b""
    b = bytearray(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), lb).astype(np.uint8)) if lb else bytearray()
    lo, hi = max(0, d), min(la, d + lb)
    for i in range(lo, hi):
        b[i - d] = a[i]
    where = rng.permutation(np.arange(lo, max(lo, hi)))[:subs]
    swap = {65: 67, 67: 71, 71: 84, 84: 65}
    for i in where.tolist():
        b[i - d] = swap.get(a[i], 65)
    return a, revcomp(profile, bytes(b))
