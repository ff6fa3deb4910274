"""UMI grouping and deduplication of a read batch (sassy_hip_umi_groups_reads, sassy_hip_dedup_reads, DeviceReads.umi_groups,
DeviceReads.dedup) restated.  The grouping is umi_groups_ref.expected_umi_groups on the list of windows, the gather is
demux_reads_ref.expected_select: this file holds no second copy of either.  All arithmetic is integer; there are no floats.

Read r of la bytes.  Its key is its window of m bytes at w: from the 5' end w = at, from the 3' end w = la - at - m; the read
has a window iff at + m <= la.  A read without a window takes no part: label = rep = 2^32 - 1, size = count = 0, never kept.
Let r_0 < r_1 < ... be the reads that have a window: the four columns, n_unique and n_groups are those of the list of their
windows, every index j of that result mapped to r_j.
The kept read of a group: the member with the highest score, on a tie the smallest index; score = the sum of the read's raw
quality bytes where the batch keeps qualities, else its length.  As one key: score << 32 | (0xFFFFFFFF - r), maximised.
kept lists the kept reads in ascending read index; record j of the deduplicated batch is read kept[j] whole."""
import numpy as np

import umi_groups_ref as uref
from demux_reads_ref import expected_select

NONE = 0xFFFFFFFF


def windows(seqs, m: int, at: int = 0, end3: bool = False):
    """(the indices r_0 < r_1 < ... of the reads that have a window, their windows)."""
    have = [r for r, s in enumerate(seqs) if at + m <= len(s)]
    wins = []
    for r in have:
        w = len(seqs[r]) - at - m if end3 else at
        wins.append(bytes(seqs[r][w:w + m]))
    return have, wins


def split(reads):
    seqs = [bytes(x[0] if isinstance(x, tuple) else x) for x in reads]
    quals = [bytes(x[1]) if isinstance(x, tuple) else None for x in reads]
    return seqs, quals


def expected_groups(profile: str, reads, m: int, k: int = 1, method: str = "directional", at: int = 0, end3: bool = False, rc: bool = False):
    """(label, size, rep, count, n_unique, n_groups); the columns uint32 with one entry per read."""
    seqs, _ = split(reads)
    n = len(seqs)
    label, rep = np.full(n, NONE, dtype=np.uint32), np.full(n, NONE, dtype=np.uint32)
    size, count = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    have, wins = windows(seqs, m, at, end3)
    if not have:
        return label, size, rep, count, 0, 0
    l, s, r, c = uref.expected_umi_groups(profile, wins, k, method, rc=rc)
    back = np.array(have, dtype=np.uint32)
    label[back], size[back], rep[back], count[back] = back[l], s, back[r], c
    return label, size, rep, count, int((r == np.arange(len(have))).sum()), int((l == np.arange(len(have))).sum())


def scores(reads):
    """Per read: the sum of its quality bytes, or its length where there are no qualities."""
    seqs, quals = split(reads)
    return [len(s) if q is None else sum(q) for s, q in zip(seqs, quals)]


def kept_of(label, score):
    """The kept read of every group, ascending: the highest key score << 32 | (0xFFFFFFFF - r) among its members."""
    best = {}
    for r, l in enumerate(np.asarray(label).tolist()):
        if l == NONE:
            continue
        key = (int(score[r]) << 32) | (0xFFFFFFFF - r)
        if key > best.get(l, 0):
            best[l] = key
    return np.array(sorted(0xFFFFFFFF - (key & 0xFFFFFFFF) for key in best.values()), dtype=np.uint64)


def expected_dedup(profile: str, reads, m: int, k: int = 1, method: str = "directional", at: int = 0, end3: bool = False, rc: bool = False):
    """(label, size, rep, count, n_unique, n_groups, kept, [(sequence, quality or None)] of the deduplicated batch)."""
    cols = expected_groups(profile, reads, m, k, method, at, end3, rc)
    kept = kept_of(cols[0], scores(reads))
    assert len(kept) == cols[5]
    return cols + (kept, expected_select(reads, kept.astype(np.int64).tolist()))


# ---- a case written out by hand (dna, m = 4 at the 5' end, k = 1, no rc): umi_groups_ref's HAND as the heads of reads ----
# The windows are umi_groups_ref.HAND with two short reads put in between (at places 3 and 9 of the batch), so every index
# behind them moves; the tails differ in length, and so do the scores (no qualities: the length).
def hand_batch():
    tails = [b"", b"C", b"GG", b"", b"TTTT", b"A", b"CCCCC", b"AA", b"", b"G", b"T", b"", b"ACGTA", b"AC", b"", b"A", b"AAAAAA", b"A"]
    reads = [w + t for w, t in zip(uref.HAND, tails)]
    reads.insert(3, b"AAA")
    reads.insert(9, b"")
    return reads


def _moved(j):  # index j of the list of windows in the batch
    return j + (1 if j >= 3 else 0) + (1 if j >= 8 else 0)


HAND_NO_WINDOW = (3, 9)
# directional groups of umi_groups_ref: {AAAA, AAAT} labelled 0, {AATT} labelled 2, {CCCC} labelled 4 (indices of the list).
# The longest read of the first group is AAAA + AAAAAA (list index 16); of {AATT}: AATT + GG (list index 2; AATT + AC ties
# at 6 bytes and is the later one); CCCC + TTTT is alone.
HAND_KEPT = {"directional": sorted(_moved(j) for j in (16, 2, 4))}


def seeded_batch(n: int, seed: int, m: int = 12, at: int = 0, end3: bool = False, with_quality: bool = True, letters: bytes = b"ACGT", rc_mix: bool = False,
                 n_umis: int = 0):
    """A seeded batch whose groups are non-trivial: about n / 8 UMIs (n_umis > 0: that many) drawn with a skewed abundance, one
    read in five carrying one substitution in its key, one in nine too short for a window (empty ones among them), one
    read in four of flat qualities and one of four lengths so that scores tie.  rc_mix: a third of the keys reverse-complemented (ACGT letters)."""
    rnd = np.random.RandomState(seed)
    pick = lambda k_: bytes(rnd.choice(np.frombuffer(letters, dtype=np.uint8), size=k_).tolist())
    n_umis = n_umis or max(1, n // 8)
    umis = [pick(m) for _ in range(n_umis)]
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    reads = []
    for r in range(n):
        if r % 9 == 8:
            la = rnd.randint(0, at + m) if rnd.randint(3) else 0
            seq = pick(la)
        else:
            u = bytearray(umis[min(rnd.randint(n_umis), rnd.randint(n_umis))])  # (the smaller of two draws: a skew)
            if r % 5 == 4:
                i = rnd.randint(m)
                u[i:i + 1] = pick(1)
            if rc_mix and r % 3 == 1:
                u = bytearray(bytes(u).translate(comp)[::-1])
            head, tail = pick(at), pick(rnd.randint(0, 40) if r % 4 else 10 * rnd.randint(0, 4))  # (few lengths where the qualities are flat: ties)
            seq = (tail + bytes(u) + head) if end3 else (head + bytes(u) + tail)
        if with_quality:
            q = bytes((np.array([35, 40, 40, 70], dtype=np.uint8)[rnd.randint(0, 4, size=len(seq))]).tolist()) if r % 4 else bytes([70]) * len(seq)
            reads.append((seq, q))
        else:
            reads.append(seq)
    return reads


def describe(profile: str, reads, m: int, k: int = 1, method: str = "directional", at: int = 0, end3: bool = False, rc: bool = False):
    """What makes a batch non-trivial, by this helper alone: groups of more than one distinct key, reads without a window, groups
    whose best score is shared."""
    label, size, rep, count, n_unique, n_groups = expected_groups(profile, reads, m, k, method, at, end3, rc)
    score = scores(reads)
    members = {}
    for r, l in enumerate(label.tolist()):
        if l != NONE:
            members.setdefault(l, []).append(r)
    mixed = sum(1 for g in members.values() if len({int(rep[r]) for r in g}) > 1)
    ties = sum(1 for g in members.values() if sum(1 for r in g if score[r] == max(score[x] for x in g)) > 1)
    return dict(n_groups=n_groups, n_unique=n_unique, mixed_groups=mixed, no_window=int((label == NONE).sum()), score_ties=ties,
                multi=sum(1 for g in members.values() if len(g) > 1))
