"""Searcher.umi_groups on the device against tests/helpers/umi_groups_ref.py (duplicates by a dict, neighbours by brute force,
`directional` as UMI-tools' sequential procedure): labels, sizes, reps and counts compared for exact equality, array to array.
The shapes are the smallest at which the collapse, the walk over the distinct sequences and the relaxation can go wrong -- the
seams of a wavefront and of a strip, a table at load 1 whose probes wrap, every word count of the planes, ties of the count
rule, a long path that needs many relaxation rounds -- not a workload."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import clusters_ref as cref  # noqa: E402
import umi_groups_ref as uref  # noqa: E402
from scan_levels import near_copy, random_rows, revcomp  # noqa: E402

pytestmark = pytest.mark.gpu

NEXT = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}
NAMES = ("labels", "sizes", "reps", "counts")


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


def groups(s, a, k, method):
    got = s.umi_groups(a, k, method)
    assert len(got) == 4 and all(col.dtype == np.uint32 and len(col) == len(a) for col in got)
    return got


def check(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.tolist() == w.tolist(), (name, what)


def check_against_helper(s, profile, rc, a, k, methods=uref.METHODS):
    out = {}
    for method in methods:
        out[method] = groups(s, a, k, method)
        check(out[method], uref.expected_umi_groups(profile, a, k, method, rc=rc), method)
    return out


def reads(rng, profile, n, m, origins, err=0.15, letters="dna"):
    """n reads of `origins` random sequences, drawn with very unequal shares (so that counts differ widely), each with one row
    changed at probability err; shuffled by construction (every read draws its origin anew)."""
    base = random_rows(rng, profile, origins, m)
    share = rng.random(origins) ** 3 + 1e-3
    pick = rng.choice(origins, size=n, p=share / share.sum())
    a = base[pick].copy()
    for i in np.flatnonzero(rng.random(n) < err):
        a[i] = near_copy(rng, letters, a[i], 1)
    return np.ascontiguousarray(a)


def listed(seqs_and_counts, rng=None):
    """[(sequence, count)] -> the rows, each sequence `count` times, interleaved round robin (or shuffled by rng)"""
    rows = []
    left = [[np.frombuffer(s, dtype=np.uint8), c] for s, c in seqs_and_counts]
    while any(c for _, c in left):
        for item in left:
            if item[1]:
                rows.append(item[0])
                item[1] -= 1
    a = np.array(rows, dtype=np.uint8)
    return np.ascontiguousarray(a if rng is None else a[rng.permutation(len(a))])


# ---------------------------------------------------------------- the hand case
def test_hand_case(sassy):
    s = sassy.Searcher("dna", rc=False)
    for method in uref.METHODS:
        labels, sizes, reps, counts = groups(s, uref.HAND, uref.HAND_K, method)
        assert reps.tolist() == uref.HAND_REPS and counts.tolist() == uref.HAND_COUNTS, method
        assert labels.tolist() == uref.HAND_LABELS[method] and sizes.tolist() == uref.HAND_SIZES[method], method
    st = s.stats()
    assert st["filtered"] == 12 and st["hit_blocks"] == 4 and st["candidates"] == 2 and st["blocks"] >= 1  # (directional ran last)


# ---------------------------------------------------------------- sizes: wavefront, strip and table seams
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 255, 256, 257, 1000))
def test_sizes_around_wave_and_strip(sassy, n):
    rng = np.random.default_rng(n)
    rc = bool(n % 2)
    a = reads(rng, "dna", n, 12, max(1, n // 4))
    if rc and n >= 4:
        a[n // 2] = revcomp("dna", a[0])
    s = sassy.Searcher("dna", rc=rc)
    out = check_against_helper(s, "dna", rc, a, 1)
    if n >= 63:  # (something was collapsed and something was joined)
        assert (out["unique"][3] > 1).any() and (out["directional"][0] != out["unique"][0]).any()


def test_all_identical(sassy):
    a = np.tile(np.frombuffer(b"ACGTACGTACGTACGT", dtype=np.uint8), (1000, 1))
    a[1::2] |= 0x20  # (lower case: the same planes under Dna)
    for forced in (0, 1000):  # the default table, and one slot per read
        s = sassy.Searcher("dna", rc=False).set_option("collapse_slots", forced)
        for method in uref.METHODS:
            labels, sizes, reps, counts = groups(s, a, 1, method)
            assert not labels.any() and not reps.any() and (sizes == 1000).all() and (counts == 1000).all()
            assert s.stats()["hit_blocks"] == 1


@pytest.mark.parametrize("n,forced", ((257, 0), (257, 257), (1000, 0), (1000, 1), (255, 300)))
def test_all_distinct_and_the_table_at_load_one(sassy, n, forced):
    """n distinct sequences (a counter written in base 4, far from sorted by hash): every slot of a table of n is taken and the
    probes wrap round; a forced size below n is raised to n.  Neighbours exist (the counter's last digit), all of count 1."""
    digits = (np.arange(n)[:, None] >> (2 * np.arange(8)[None, :])) & 3
    a = np.ascontiguousarray(np.frombuffer(b"ACGT", dtype=np.uint8)[digits][np.random.default_rng(n).permutation(n)])
    s = sassy.Searcher("dna", rc=False).set_option("collapse_slots", forced)
    out = check_against_helper(s, "dna", False, a, 1)
    assert out["unique"][2].tolist() == list(range(n)) and (out["unique"][3] == 1).all()
    assert not out["directional"][0].any() and not out["cluster"][0].any()  # (the counter's graph is connected)


def test_the_only_duplicate_of_entry_0_in_the_last_place(sassy):
    rng = np.random.default_rng(7)
    a = random_rows(rng, "dna", 600, 20)
    a[-1] = a[0]
    s = sassy.Searcher("dna", rc=False)
    out = check_against_helper(s, "dna", False, a, 2)
    assert out["unique"][2][-1] == 0 and out["unique"][3][0] == 2 and out["unique"][3][-1] == 2 and (out["unique"][3][1:-1] == 1).all()


# ---------------------------------------------------------------- alphabets x plane words
@pytest.mark.parametrize("m", (1, 16, 32, 33, 64, 65, 128))
@pytest.mark.parametrize("profile", ("dna", "iupac", "ascii", "ascii_ci"))
def test_alphabets_and_word_counts(sassy, profile, m):
    """every P x W of the planes.  iupac: N among the letters (it matches everything and is a duplicate of nothing but N);
    ascii_ci: every second read or so with the case of all its letters swapped, so reads fold to duplicates that ascii keeps apart"""
    rng = np.random.default_rng(m * 7 + len(profile))
    n = 300
    a = reads(rng, profile, n, m, 40, letters=profile)
    if profile.startswith("ascii"):
        letter = ((a | 0x20) >= ord("a")) & ((a | 0x20) <= ord("z"))
        a = np.where(letter & (rng.random((n, 1)) < 0.5), a ^ 0x20, a).astype(np.uint8)
    a = np.ascontiguousarray(a)
    rc = profile in ("dna", "iupac") and m % 2 == 0
    s = sassy.Searcher(profile, rc=rc)
    out = check_against_helper(s, profile, rc, a, 1 if m > 1 else 0)
    n_u = int((out["unique"][2] == np.arange(n)).sum())
    assert n_u < n
    if profile == "ascii_ci" and m >= 16:  # (folding made duplicates that plain ascii does not see)
        plain = sassy.Searcher("ascii", rc=False).umi_groups(a, 1, "unique")
        assert int((plain[2] == np.arange(n)).sum()) > n_u


def test_iupac_n_matches_and_is_no_duplicate(sassy):
    a = [b"ACGN", b"ACGA", b"acgn", b"ACGT", b"ACGA"]
    s = sassy.Searcher("iupac", rc=False)
    labels, sizes, reps, counts = groups(s, a, 0, "cluster")
    assert (labels.tolist(), sizes.tolist(), reps.tolist(), counts.tolist()) == ([0] * 5, [5] * 5, [0, 1, 0, 3, 1], [2, 2, 2, 1, 2])
    check_against_helper(s, "iupac", False, a, 0)


# ---------------------------------------------------------------- cluster == hamming_clusters
@pytest.mark.parametrize("k", (0, 1, 2, 12, 254))
def test_cluster_method_equals_hamming_clusters(sassy, k):
    """the yardstick that exists already: method="cluster" gives the labels and sizes of Searcher.hamming_clusters on the same
    list, and both equal clusters_ref on the full list (k = m and k = 254: one cluster)"""
    rng = np.random.default_rng(100 + k)
    for rc in (False, True):
        a = reads(rng, "dna", 700, 12, 120)
        s = sassy.Searcher("dna", rc=rc)
        labels, sizes, _, _ = groups(s, a, k, "cluster")
        own = s.hamming_clusters(a, k)
        want = cref.expected_clusters("dna", a, k, rc=rc)
        assert labels.tolist() == own[0].tolist() == want[0].tolist()
        assert sizes.tolist() == own[1].tolist() == want[1].tolist()
        if k >= 12:
            assert not labels.any() and (sizes == 700).all()


@pytest.mark.parametrize("k", (0, 5))
def test_unique_is_label_equals_rep(sassy, k):
    a = reads(np.random.default_rng(k), "dna", 500, 10, 30)
    s = sassy.Searcher("dna", rc=False)
    labels, sizes, reps, counts = groups(s, a, k, "unique")
    assert labels.tolist() == reps.tolist() and sizes.tolist() == counts.tolist()
    check((labels, sizes, reps, counts), uref.expected_umi_groups("dna", a, k, "unique"))
    st = s.stats()
    assert st["candidates"] == 0 and st["hit_blocks"] == int((reps == np.arange(500)).sum())


# ---------------------------------------------------------------- directional: the count rule at its edges
def test_equal_counts_the_tie_goes_to_the_smaller_index(sassy):
    s = sassy.Searcher("dna", rc=False)
    for first, second in ((b"AAAT", b"AAAA"), (b"AAAA", b"AAAT")):
        # count 1 on both sides: they point at each other, index 0 opens
        assert groups(s, [first, second], 1, "directional")[0].tolist() == [0, 0]
        # count 2 on both sides: 2 < 2 * 2 - 1, no edge either way
        assert groups(s, [first, second, first, second], 1, "directional")[0].tolist() == [0, 1, 0, 1]
        check_against_helper(s, "dna", False, [first, second, first, second], 1)
    # three of count 1 in a row: whichever stands first opens and takes the others, through the middle one where it must
    check_against_helper(s, "dna", False, [b"AAAT", b"AAAA", b"AATT"], 1)
    assert groups(s, [b"AATT", b"AAAA", b"AAAT"], 1, "directional")[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("c_v", (2, 4, 9))
def test_count_rule_exactly_at_and_one_below_the_threshold(sassy, c_v):
    s = sassy.Searcher("dna", rc=False)
    for c_u, joined in ((2 * c_v - 1, True), (2 * c_v - 2, False)):
        for rare_first in (False, True):
            pair = [(b"ACGTACGA", c_v), (b"ACGTACGT", c_u)] if rare_first else [(b"ACGTACGT", c_u), (b"ACGTACGA", c_v)]
            a = listed(pair)
            labels, sizes, reps, counts = check_against_helper(s, "dna", False, a, 1)["directional"]
            abundant = 1 if rare_first else 0
            if joined:
                assert (labels == abundant).all() and (sizes == c_u + c_v).all()
            else:
                assert labels.tolist() == reps.tolist() and sizes.tolist() == counts.tolist()


def test_reversed_path_of_129_needs_many_rounds(sassy):
    """s_t = s_0 with its first t rows changed, t = 0 .. 128, m = 128: only consecutive ones are within 1.  All of count 1, so
    every edge runs both ways and the whole path is one group, opened by index 0 -- which the reversed listing puts at the far
    end of the path, 128 edges away from the last index; then the same path shuffled"""
    rng = np.random.default_rng(129)
    s0 = random_rows(rng, "dna", 1, 128)[0]
    seq = np.tile(s0, (129, 1))
    for t in range(1, 129):
        seq[t, :t] = [NEXT[int(c)] for c in s0[:t]]
    s = sassy.Searcher("dna", rc=False)
    for a in (np.ascontiguousarray(seq[::-1]), np.ascontiguousarray(seq[rng.permutation(129)])):
        labels, sizes, reps, counts = check_against_helper(s, "dna", False, a, 1)["directional"]
        assert not labels.any() and (sizes == 129).all() and reps.tolist() == list(range(129))
        st = s.stats()
        assert st["candidates"] == 128 and 2 <= st["blocks"] <= 130
    # the same path with falling counts from one end: every edge runs one way, and still one group, opened by the abundant end
    a = listed([(seq[t].tobytes(), 1 << (7 - t)) for t in range(8)], rng)
    labels = check_against_helper(s, "dna", False, a, 1)["directional"][0]
    assert len(set(labels.tolist())) == 1
    # rising towards the middle: two slopes, one opener
    a = listed([(seq[t].tobytes(), 1 << (4 - abs(t - 4))) for t in range(9)], rng)
    assert len(set(check_against_helper(s, "dna", False, a, 1)["directional"][0].tolist())) == 1


@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_star_with_an_abundant_hub(sassy, where):
    """a hub of 40 reads and 120 spokes of 1 .. 3 reads, each one change from the hub (and two from each other): directional and
    cluster both give one group, labelled by the hub's first read wherever it stands -- the spokes before it included"""
    rng = np.random.default_rng(len(where))
    hub = random_rows(rng, "dna", 1, 128)[0]
    spokes = []
    for t in range(120):
        row = hub.copy()
        row[t] = NEXT[int(row[t])]
        spokes += [row] * (1 + t % 3)
    spokes = np.array(spokes, dtype=np.uint8)[rng.permutation(len(spokes))]
    at = {"first": 0, "middle": len(spokes) // 2, "last": len(spokes)}[where]
    a = np.ascontiguousarray(np.concatenate([spokes[:at], np.tile(hub, (40, 1)), spokes[at:]]))
    s = sassy.Searcher("dna", rc=False)
    out = check_against_helper(s, "dna", False, a, 1)
    assert (out["directional"][0] == at).all() and (out["directional"][1] == len(a)).all()
    assert (out["cluster"][0] == 0).all()
    # a rare hub between two abundant spokes absorbs nothing and is absorbed by both: the first of them in the order takes it
    first, second = hub.copy(), hub.copy()
    first[0], second[1] = NEXT[int(hub[0])], NEXT[int(hub[1])]
    a = listed([(hub.tobytes(), 2), (first.tobytes(), 20), (second.tobytes(), 20)], rng)
    labels = check_against_helper(s, "dna", False, a, 1)["directional"][0]
    assert len(set(labels.tolist())) == 2


def test_rc_searcher_reverse_complements_and_palindromes(sassy):
    rng = np.random.default_rng(11)
    base = random_rows(rng, "dna", 30, 16)
    rows = []
    for i, row in enumerate(base):
        rows += [row] * (1 + i % 5)
        rows += [revcomp("dna", near_copy(rng, "dna", row, i % 2))] * (1 + i % 3)   # the other strand, half of them one change off
    half = random_rows(rng, "dna", 6, 8)
    rows += [np.concatenate([h, revcomp("dna", h)]) for h in half] * 2           # palindromes: (u, u, 1) is a record and no edge
    a = np.ascontiguousarray(np.array(rows, dtype=np.uint8)[rng.permutation(len(rows))])
    for rc in (True, False):
        out = check_against_helper(sassy.Searcher("dna", rc=rc), "dna", rc, a, 1)
        if rc:
            joined = out["directional"][0]
        else:
            assert (out["directional"][0] != joined).any()   # (the strands fall apart without rc)


# ---------------------------------------------------------------- geometry: chunks, twice over
@pytest.mark.parametrize("chunks", (1, 3, 7, 0))
def test_reads_with_errors_under_every_chunking_twice(sassy, chunks):
    rng = np.random.default_rng(4001)
    a = reads(rng, "dna", 4001, 14, 40, err=0.2)
    s = sassy.Searcher("dna", rc=False).set_option("pairs_chunks", chunks)
    want = {method: uref.expected_umi_groups("dna", a, 1, method) for method in ("cluster", "directional")}
    for method in ("cluster", "directional"):
        first = groups(s, a, 1, method)
        again = groups(s, a, 1, method)
        check(first, want[method], method)
        check(again, first, method + ", the second run")
        st = s.stats()
        assert 1 <= st["chunks"] <= (chunks or st["chunks"]) and (chunks != 1 or st["chunks"] == 1)
    assert (want["directional"][0] != want["cluster"][0]).any()   # (the count rule keeps apart what the components join)


def test_50000_reads_of_500_origins(sassy):
    rng = np.random.default_rng(50000)
    a = reads(rng, "dna", 50000, 16, 500, err=0.04)
    s = sassy.Searcher("dna", rc=False)
    want = uref.expected_umi_groups("dna", a, 1, "directional")
    got = groups(s, a, 1, "directional")
    check(got, want)
    n_u = int((want[2] == np.arange(50000)).sum())
    st = s.stats()
    assert 500 < n_u < 5000 and st["hit_blocks"] == n_u and st["candidates"] > n_u - 500
    labels, sizes = s.hamming_clusters(a, 1)
    cluster = groups(s, a, 1, "cluster")
    assert cluster[0].tolist() == labels.tolist() and cluster[1].tolist() == sizes.tolist()
