"""Searcher.hamming_clusters / edit_clusters on the device against tests/helpers/clusters_ref.py (the brute-force pair
records of the helpers, unioned by a plain union-find): labels and sizes compared for exact equality, array to array.  The
shapes are the smallest at which the link kernels can go wrong -- the seams of a wavefront (64 entries), of a strip (256), of
a chunk of targets; long chases and racing hooks (a shuffled path), one contended root (a star), the already-joined branch on
every hit (a clique) -- not a workload."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import oracle  # noqa: E402
import clusters_ref as cref  # noqa: E402
from scan_levels import near_copy, random_rows  # noqa: E402

pytestmark = pytest.mark.gpu

CALLS = ("hamming", "edit")
NEXT = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


def clusters(s, call, a, k):
    labels, sizes = (s.edit_clusters if call == "edit" else s.hamming_clusters)(a, k)
    assert labels.dtype == np.uint32 and sizes.dtype == np.uint32 and len(labels) == len(sizes) == len(a)
    return labels, sizes


def check(got, want):
    assert got[0].tolist() == want[0].tolist()
    assert got[1].tolist() == want[1].tolist()


def check_against_helper(s, profile, rc, call, a, k):
    got = clusters(s, call, a, k)
    check(got, cref.expected_clusters(profile, a, k, rc=rc, edit=call == "edit"))
    return got


def families(rng, profile, n, m, k, share=0.6, size=5):
    """n rows: `share` of them in families -- a random centre and members with 0 .. k rows of it changed (members of one family
    lie within 2 k of each other: some joined directly, some through the centre, some not at all) --, the rest random
    singletons; all of it shuffled."""
    a = random_rows(rng, profile, n, m)
    i = 0
    while i < int(n * share):
        centre = random_rows(rng, "dna", 1, m)[0]
        for q in range(min(int(rng.integers(2, 2 * size)), n - i)):
            a[i] = near_copy(rng, "dna", centre, int(rng.integers(0, k + 1)) if q else 0)
            i += 1
    return np.ascontiguousarray(a[rng.permutation(n)])


# ---------------------------------------------------------------- strip and wavefront borders
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 255, 256, 257, 513))
def test_strip_and_wave_borders(sassy, n):
    """every size around a wavefront and a strip, both calls, with and without rc: copies of one sequence at 0 .. 2 changes sit
    on both sides of every seam, so that edges cross every border of the grid"""
    rng = np.random.default_rng(n)
    for q, call in enumerate(CALLS):
        rc = bool((n + q) % 2)
        a = random_rows(rng, "dna", n, 12)
        base = random_rows(rng, "dna", 1, 12)[0]
        for t, i in enumerate(i for i in (0, 1, 62, 63, 64, 65, 127, 128, 254, 255, 256, 257, 511, 512) if i < n):
            a[i] = near_copy(rng, "dna", base, t % 3)
            if rc and t % 4 == 3:
                a[i] = np.frombuffer(oracle.reverse_complement("dna", a[i].tobytes()), dtype=np.uint8)
        s = sassy.Searcher("dna", rc=rc)
        labels, _ = check_against_helper(s, "dna", rc, call, a, 1)
        if n >= 2:  # (something was joined: entries 0 and 1 are one change apart)
            assert labels[1] == 0 and (labels != np.arange(n)).sum() >= (4 if n >= 257 else 1)


# ---------------------------------------------------------------- a shuffled path: deep chases, racing hooks
def path(rng, n, m, break_at=None):
    """seq[t + 1] = seq[t] with position t mod m stepped to the next letter (break_at: that step changes two positions), the
    indices permuted: H(seq[t], seq[t + d]) = d for d <= m, and at least 2 for every d >= 2 while n < 4 m"""
    assert n < 4 * m
    seq = np.empty((n, m), dtype=np.uint8)
    seq[0] = random_rows(rng, "dna", 1, m)[0]
    for t in range(n - 1):
        seq[t + 1] = seq[t]
        seq[t + 1, t % m] = NEXT[int(seq[t, t % m])]
        if t == break_at:
            seq[t + 1, (t + m // 2) % m] = NEXT[int(seq[t, (t + m // 2) % m])]
    order = rng.permutation(n)
    out = np.empty_like(seq)
    out[order] = seq  # path position t sits at index order[t]
    return out, order


@pytest.mark.parametrize("call,n,m", (("hamming", 500, 128), ("hamming", 120, 33), ("edit", 250, 64), ("edit", 90, 31)))
def test_shuffled_path_is_one_component(sassy, call, n, m):
    rng = np.random.default_rng(n + m)
    s = sassy.Searcher("dna", rc=False)
    a, _ = path(rng, n, m)
    labels, sizes = check_against_helper(s, "dna", False, call, a, 1)
    assert not labels.any() and (sizes == n).all()  # (index 0 is the smallest of the one component, wherever it sits)
    assert (clusters(s, call, a, 0)[0] == np.arange(n)).all()
    # one step of two changes: exactly two components, each rooted at the smallest index of its side
    cut = n // 3
    a, order = path(rng, n, m, break_at=cut)
    labels, sizes = check_against_helper(s, "dna", False, call, a, 1)
    left, right = order[:cut + 1], order[cut + 1:]
    assert (labels[left] == left.min()).all() and (labels[right] == right.min()).all()
    assert (sizes[left] == cut + 1).all() and (sizes[right] == n - cut - 1).all()


# ---------------------------------------------------------------- a star: every link goes for one root
@pytest.mark.parametrize("call,m", (("hamming", 128), ("edit", 64)))
def test_star_around_a_hub(sassy, call, m):
    """a hub and 3 m leaves, each one substitution from the hub at a (position, letter) of its own: leaves are two apart, so
    at k = 1 every edge has the hub at one end; hub first, in the middle, last"""
    rng = np.random.default_rng(m)
    hub = random_rows(rng, "dna", 1, m)[0]
    leaves = []
    for t in range(m):
        for c in b"ACGT":
            if c != hub[t]:
                leaf = hub.copy()
                leaf[t] = c
                leaves.append(leaf)
    leaves = np.array(leaves)[rng.permutation(3 * m)]
    n = 3 * m + 1
    s = sassy.Searcher("dna", rc=False)
    for at in (0, n // 2, n - 1):
        a = np.ascontiguousarray(np.insert(leaves, at, hub, axis=0))
        labels, sizes = check_against_helper(s, "dna", False, call, a, 1)
        assert not labels.any() and (sizes == n).all()
        assert (clusters(s, call, a, 0)[0] == np.arange(n)).all()


# ---------------------------------------------------------------- cliques: the already-joined branch on every hit
@pytest.mark.parametrize("call", CALLS)
def test_cliques_of_identical_sequences(sassy, call):
    rng = np.random.default_rng(7)
    s = sassy.Searcher("dna", rc=False)
    same = np.repeat(random_rows(rng, "dna", 1, 16), 1000, axis=0)
    for k in (0, 1):
        labels, sizes = clusters(s, call, same, k)
        assert not labels.any() and (sizes == 1000).all()
    # 1000 copies of 10 centres that are far apart (the helper agrees that they are)
    centres = random_rows(rng, "dna", 10, 20)
    which = rng.integers(0, 10, size=1000)
    a = np.ascontiguousarray(centres[which])
    labels, sizes = check_against_helper(s, "dna", False, call, a, 1)
    first = np.array([np.flatnonzero(which == c)[0] for c in range(10)])
    assert labels.tolist() == first[which].tolist() and sorted(set(labels.tolist())) == sorted(first.tolist())


# ---------------------------------------------------------------- many small clusters, and the chunks' borders
def test_many_small_clusters_and_chunk_borders(sassy):
    """about 4000 sequences of 16 bases in families and singletons: the default plan spans several chunks; every forced chunk
    count and a second call give the same arrays"""
    rng = np.random.default_rng(11)
    a = families(rng, "dna", 4001, 16, 2)
    want = cref.expected_clusters("dna", a, 2)
    assert 500 < (want[0] == np.arange(len(a))).sum() < 3500 and want[1].max() >= 4
    s = sassy.Searcher("dna", rc=False)
    got = clusters(s, "hamming", a, 2)
    check(got, want)
    st = s.stats()
    assert st["filtered"] == 10 and st["chunks"] > 1 and st["grid"] == 16
    for chunks in (1, 3, 7, 64):
        forced = sassy.Searcher("dna", rc=False)
        forced.set_option("pairs_chunks", chunks)
        check(clusters(forced, "hamming", a, 2), want)
        assert forced.stats()["chunks"] == chunks
        check(clusters(forced, "hamming", a, 2), want)  # (the same call again)
    check(clusters(s, "hamming", a, 2), want)


def test_many_small_clusters_under_the_edit_distance(sassy):
    rng = np.random.default_rng(13)
    a = families(rng, "dna", 1100, 16, 1)
    for i in range(0, 1100, 9):  # some members lose their first base and gain one at the end
        a[i] = np.r_[a[(i + 1) % 1100][1:], a[i][:1]]
    want = cref.expected_clusters("dna", a, 2, edit=True)
    s = sassy.Searcher("dna", rc=False)
    check(clusters(s, "edit", a, 2), want)
    st = s.stats()
    assert st["filtered"] == 11 and st["chunks"] > 1
    for chunks in (1, 3, 7, 64):
        forced = sassy.Searcher("dna", rc=False)
        forced.set_option("pairs_chunks", chunks)
        check(clusters(forced, "edit", a, 2), want)
        check(clusters(forced, "edit", a, 2), want)


# ---------------------------------------------------------------- profiles and word counts
@pytest.mark.parametrize("profile", ("dna", "iupac", "ascii", "ascii_ci"))
def test_profiles_and_word_counts(sassy, profile):
    rng = np.random.default_rng(len(profile))
    for call, ms in (("hamming", (1, 32, 33, 64, 65, 128)), ("edit", (1, 31, 32, 33, 63, 64))):
        for q, m in enumerate(ms):
            rc = profile in ("dna", "iupac") and q % 2 == 1
            k = min(2, m - 1) if m > 1 else 0
            a = random_rows(rng, profile, 150, m)
            base = random_rows(rng, profile, 1, m)[0]
            for i in range(0, 150, 3):
                a[i] = near_copy(rng, profile, base if i % 2 else a[(i + 7) % 150], int(rng.integers(0, k + 2)))
            if profile == "ascii_ci":
                a[1::6] = np.frombuffer(a[1::6].tobytes().swapcase(), dtype=np.uint8).reshape(a[1::6].shape)
            s = sassy.Searcher(profile, rc=rc)
            check_against_helper(s, profile, rc, call, np.ascontiguousarray(a), k)


@pytest.mark.parametrize("call", CALLS)
def test_relations_of_the_profiles(sassy, call):
    # Iupac: an all-N sequence meets everything at k = 0 -- one cluster, though ACGT and TTTT are four apart
    a = [b"ACGT", b"TTTT", b"GGCC", b"NNNN", b"CATG"]
    labels, sizes = clusters(sassy.Searcher("iupac", rc=False), call, a, 0)
    assert labels.tolist() == [0] * 5 and sizes.tolist() == [5] * 5
    labels, _ = clusters(sassy.Searcher("iupac", rc=False), call, a[:3] + a[4:], 0)
    assert labels.tolist() == [0, 1, 2, 3]
    # lower and upper case join under Dna and ascii_ci, not under Ascii
    a = [b"ACGTAC", b"acgtac", b"TTGTAC", b"ttgtac", b"AcGtAc"]
    for profile, want in (("dna", [0, 0, 2, 2, 0]), ("ascii_ci", [0, 0, 2, 2, 0]), ("ascii", [0, 1, 2, 3, 4])):
        got = clusters(sassy.Searcher(profile, rc=False), call, a, 0)
        assert got[0].tolist() == want, profile
        check(got, cref.expected_clusters(profile, a, 0, edit=call == "edit"))


# ---------------------------------------------------------------- strands
@pytest.mark.parametrize("call", CALLS)
def test_strands(sassy, call):
    rng = np.random.default_rng(17)
    x = random_rows(rng, "dna", 1, 20)[0]
    y = near_copy(rng, "dna", np.frombuffer(oracle.reverse_complement("dna", x.tobytes()), dtype=np.uint8), 1)
    half = random_rows(rng, "dna", 1, 10)[0].tobytes()
    palindrome = np.frombuffer(half + oracle.reverse_complement("dna", half), dtype=np.uint8)  # (i, i, 1) at cost 0: no edge
    a = np.ascontiguousarray(np.stack([random_rows(rng, "dna", 1, 20)[0], x, palindrome, y]))
    labels, sizes = check_against_helper(sassy.Searcher("dna", rc=True), "dna", True, call, a, 1)
    assert labels.tolist() == [0, 1, 2, 1] and sizes.tolist() == [1, 2, 1, 2]
    labels, sizes = check_against_helper(sassy.Searcher("dna", rc=False), "dna", False, call, a, 1)
    assert labels.tolist() == [0, 1, 2, 3] and sizes.tolist() == [1, 1, 1, 1]
    # across a strip's border too
    big = random_rows(rng, "dna", 300, 20)
    big[3], big[290] = x, y
    labels, _ = check_against_helper(sassy.Searcher("dna", rc=True), "dna", True, call, big, 1)
    assert labels[290] == 3
    assert clusters(sassy.Searcher("dna", rc=False), call, big, 1)[0][290] == 290


# ---------------------------------------------------------------- what only the edit distance joins
def test_indels_join_under_the_edit_distance_only(sassy):
    rng = np.random.default_rng(19)
    s = sassy.Searcher("dna", rc=False)
    for m in (16, 40, 64):
        # (no two neighbours alike: the shifted copy mismatches everywhere)
        base = np.frombuffer(b"ACGT", dtype=np.uint8)[np.cumsum(rng.integers(1, 4, size=m)) % 4]
        shifted = np.r_[base[1:], [NEXT[int(base[-1])]]].astype(np.uint8)  # one base lost at the front, one gained at the end
        a = np.ascontiguousarray(np.stack([random_rows(rng, "dna", 1, m)[0], base, random_rows(rng, "dna", 1, m)[0], shifted]))
        got = check_against_helper(s, "dna", False, "edit", a, 2)
        assert got[0].tolist() == [0, 1, 2, 1] and got[1].tolist() == [1, 2, 1, 2]
        got = check_against_helper(s, "dna", False, "hamming", a, 2)
        assert got[0].tolist() == [0, 1, 2, 3]
        assert clusters(s, "edit", a, 1)[0].tolist() == [0, 1, 2, 3]
    # k = 1, equal lengths: one edit is one substitution, the two calls agree
    a = families(rng, "dna", 700, 16, 1)
    check(clusters(s, "edit", a, 1), clusters(s, "hamming", a, 1))
    check_against_helper(s, "dna", False, "hamming", a, 1)


# ---------------------------------------------------------------- k
@pytest.mark.parametrize("call", CALLS)
def test_k_zero_k_beyond_m_and_the_largest_k(sassy, call):
    rng = np.random.default_rng(23)
    a = random_rows(rng, "dna", 300, 12)
    a[40], a[299] = a[7], a[7]
    s = sassy.Searcher("dna", rc=False)
    labels, sizes = check_against_helper(s, "dna", False, call, a, 0)
    assert labels[40] == 7 and labels[299] == 7 and sizes[7] >= 3
    for k in (12, 13, 254):  # k >= m: every pair is an edge
        labels, sizes = clusters(s, call, a, k)
        assert not labels.any() and (sizes == 300).all()
    far = np.ascontiguousarray(np.stack([np.full(64, ord("A"), dtype=np.uint8), np.full(64, ord("C"), dtype=np.uint8)]))
    assert clusters(s, call, far, 63)[0].tolist() == [0, 1] and clusters(s, call, far, 64)[0].tolist() == [0, 0]


# ---------------------------------------------------------------- a size brute force cannot take
@pytest.mark.parametrize("call", CALLS)
def test_labels_are_the_components_of_the_pair_records(sassy, call):
    """50 000 random 16-mers with planted families: the labels equal the components of the project's own self-mode pair
    records (which the pair calls' tests tie to brute force), unioned on the host"""
    rng = np.random.default_rng(29)
    a = families(rng, "dna", 50000, 16, 1, share=0.3, size=6)
    s = sassy.Searcher("dna", rc=False)
    k = 2 if call == "hamming" else 1
    records = (s.edit_pairs if call == "edit" else s.hamming_pairs)(a, None, k)
    assert len(records) > 20000
    want = cref.components_fast(len(a), records["a_idx"], records["b_idx"])
    labels, sizes = clusters(s, call, a, k)
    assert labels.tolist() == want.tolist()
    assert sizes.tolist() == np.bincount(want, minlength=len(a))[want].tolist()
    assert 1000 < (labels != np.arange(len(a))).sum() and s.stats()["chunks"] > 1


# ---------------------------------------------------------------- the `cluster` verb
def test_cli_cluster_rows(sassy, tmp_path, capsys):
    from sassy_amd import cli
    a = tmp_path / "a.fa"
    a.write_bytes(b"".join(b">u%d\n%s\n" % (i + 1, seq) for i, seq in enumerate(cref.HAND)))
    assert cli.main(["cluster", str(a), "-k", "1", "--rc"]) == 0
    assert capsys.readouterr().out == "id\tcluster_id\tcluster_size\nu1\tu1\t3\nu2\tu1\t3\nu3\tu1\t3\nu4\tu4\t2\nu5\tu4\t2\n"
    assert cli.main(["cluster", str(a), "-k", "1"]) == 0
    assert capsys.readouterr().out == "id\tcluster_id\tcluster_size\nu1\tu1\t3\nu2\tu1\t3\nu3\tu1\t3\nu4\tu4\t1\nu5\tu5\t1\n"
    lines = tmp_path / "b.txt"
    lines.write_bytes(b"ACGT\nCGTA\nTTTT\n")
    assert cli.main(["cluster", str(lines), "-k", "2", "--edit"]) == 0
    assert capsys.readouterr().out == "id\tcluster_id\tcluster_size\n1\t1\t2\n2\t1\t2\n3\t3\t1\n"
