"""Searcher.hamming_pairs / hamming_nearest at the sizes that enter the upper levels of their device code, which no forced
geometry reaches: more than one block of the row scan (2048 rows), more than 1024 blocks (the top scan's second turn), lists
long enough for the threaded encode (65 536 sequences), and more target records than a staged LDS tile holds.  Inputs and
sizes come from tests/helpers/scan_levels.py (tests/test_scan_levels_cpu.py keeps them beyond the kernels' thresholds); the
expectation is tests/helpers/hamming_pairs_ref.py, compared record for record, order included."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import hamming_pairs_ref as pref  # noqa: E402
import scan_levels as lv  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


def check_pairs(got, want):
    """records equal, in order; on a mismatch: the first differing record, its row and the row's scan block"""
    n = min(len(got), len(want))
    bad = np.zeros(n, dtype=bool)
    for f in ("a_idx", "b_idx", "strand", "cost"):
        bad |= got[f][:n] != want[f][:n]
    at = int(np.flatnonzero(bad)[0]) if bad.any() else n
    if at < max(len(got), len(want)):
        row = int(want["a_idx"][at]) if at < len(want) else int(got["a_idx"][at])
        pytest.fail(f"record {at} of {len(got)} (want {len(want)}): got {got[at] if at < len(got) else None}, want "
                    f"{want[at] if at < len(want) else None}; row {row} lies in scan block {row // lv.SCAN_BLOCK}")
    assert not got["pad_"].any()


def check_nearest(got, want):
    for g, w, name in zip(got, want, ("cost", "index", "strand", "ties")):
        bad = np.flatnonzero(g != w)
        assert g.dtype == w.dtype and not bad.size, (name, "row", int(bad[0]), "scan block", int(bad[0]) // lv.SCAN_BLOCK, int(g[bad[0]]), int(w[bad[0]]))


def rows_of_blocks(want, n_a, last_row_empty=False):
    """the records per row; every scan block holds empty and non-empty rows (a block of one row: that row, but for the last
    row of a triangle without rc, which is empty)"""
    per_row = np.bincount(want["a_idx"], minlength=n_a)
    for b0 in range(0, n_a, lv.SCAN_BLOCK):
        block = per_row[b0:b0 + lv.SCAN_BLOCK]
        if len(block) == 1:
            assert bool(block[0]) != last_row_empty, b0
        else:
            assert block.any() and not block.all(), b0
    return per_row


# ---------------------------------------------------------------- the row scan: two and three blocks
@pytest.mark.parametrize("n_a", lv.PAIRS_BLOCK_SIZES)
@pytest.mark.parametrize("profile", ("dna", "iupac", "ascii"))
def test_rows_beyond_one_scan_block_two_sets(sassy, profile, n_a):
    """n_a = 2047, 2048, 2049, 4097: pairs_scan_sums_kernel and pairs_scan_rows_kernel with one, one full, two and three
    blocks (n_blocks = ceil(n_a / 2048)), block_first[] non-zero from block 1 on"""
    a, b, k = lv.pairs_block_case(profile, n_a, seed=n_a)
    want = pref.expected_pairs(profile, a, b, k)
    per_row = rows_of_blocks(want, n_a)
    assert per_row[lv.block_borders(n_a)].all()
    s = sassy.Searcher(profile, rc=False)
    got = s.hamming_pairs(a, b, k)
    print(f"{profile} n_a={n_a} n_blocks={-(-n_a // lv.SCAN_BLOCK)} records={len(got)} want={len(want)} empty rows={int((per_row == 0).sum())}")
    check_pairs(got, want)
    check_nearest(s.hamming_nearest(a, b, k), lv.nearest_fast(want, n_a))


@pytest.mark.parametrize("profile,rc,n", [("dna", True, 2049), ("dna", True, 4097), ("iupac", True, 2049), ("dna", False, 4097)])
def test_rows_beyond_one_scan_block_self_mode(sassy, profile, rc, n):
    """the triangle over two and three scan blocks; without rc the last row of a triangle holds no record"""
    a, k = lv.pairs_self_case(profile, rc, n, seed=n + rc)
    want, square = pref.expected_self(profile, a, k, rc)
    per_row = rows_of_blocks(want, n, last_row_empty=not rc)
    assert per_row[[i for i in lv.block_borders(n) if 0 < i and (rc or i < n - 1)]].all()
    s = sassy.Searcher(profile, rc=rc)
    got = s.hamming_pairs(a, None, k)
    print(f"{profile} rc={rc} n={n} n_blocks={-(-n // lv.SCAN_BLOCK)} records={len(got)} want={len(want)} empty rows={int((per_row == 0).sum())}")
    check_pairs(got, want)
    check_nearest(s.hamming_nearest(a, None, k), lv.nearest_fast(square, n))


# ---------------------------------------------------------------- the top scan's second turn, the threaded encode of a
@pytest.mark.parametrize("rc", (False, True))
def test_rows_beyond_1024_scan_blocks(sassy, rc):
    """n_a = 2048 * 1024 + 2048 + 5: 1026 scan blocks, so pairs_scan_top_kernel takes a second turn of its loop over 1024
    blocks and adds the running base to blocks 1024 and 1025; encode_list encodes list a in threads"""
    a, b, k = lv.pairs_top_case()
    n_a = len(a)
    want = pref.expected_pairs("dna", a, b, k, rc)
    per_row = rows_of_blocks(want, n_a)
    assert per_row[lv.block_borders(n_a)].all() and 200_000 < len(want) < 4_000_000
    assert {0, 2047, 2048, 1024 * 2048 - 1, 1024 * 2048, n_a - 1} <= set(lv.block_borders(n_a))
    s = sassy.Searcher("dna", rc=rc)
    got = s.hamming_pairs(a, b, k)
    print(f"rc={rc} n_a={n_a} n_blocks={-(-n_a // lv.SCAN_BLOCK)} records={len(got)} want={len(want)} empty rows={int((per_row == 0).sum())}")
    check_pairs(got, want)
    check_nearest(s.hamming_nearest(a, b, k), lv.nearest_fast(want, n_a))


# ---------------------------------------------------------------- the threaded encode of the targets
@pytest.mark.parametrize("profile", ("dna", "iupac"))
def test_threaded_encode_of_the_targets(sassy, profile):
    """n_b = 70 001 >= 65 536 with rc: encode_list in slices [n w / 8, n (w + 1) / 8), each target's reverse complement
    at record 2 j + 1; near-copies and reverse complements on both sides of every slice border"""
    a, b, k = lv.encode_case(profile, seed=7)
    want = pref.expected_pairs(profile, a, b, k, True)
    hit = set(want["b_idx"][want["a_idx"] == 0].tolist())
    assert all(j in hit for q, j in enumerate(lv.encode_borders()) if q % (k + 2) <= k), sorted(hit)[:40]
    assert {0, 1}.issubset(set(want["strand"].tolist()))
    s = sassy.Searcher(profile, rc=True)
    got = s.hamming_pairs(a, b, k)
    print(f"{profile} n_b={len(b)} records={len(got)} want={len(want)}")
    check_pairs(got, want)
    want_nearest = pref.nearest_of_pairs(want, len(a))
    check_nearest(lv.nearest_fast(want, len(a)), want_nearest)
    check_nearest(s.hamming_nearest(a, b, k), want_nearest)


# ---------------------------------------------------------------- the staged tiles of the walk
SEAM_RUNS = [(case, rc) for case in lv.SEAM_CASES for rc in ((False, True) if case[0] != "ascii" else (False,))]
# per case, from pairs_walk: T = 2048 / (P W) records per staged tile, U = 8 if P W <= 4 else 32 / (P W) records per round
#   dna   m 20 (P 2, W 1): T 1024, U 8     dna   m 40 (W 2): T 512, U 8     dna   m 100 (W 4): T 256, U 4
#   iupac m 20 (P 4, W 1): T  512, U 8     iupac m 40 (W 2): T 256, U 4     iupac m 100 (W 4): T 128, U 2
#   ascii m 20 (P 8, W 1): T  256, U 4     ascii m 40 (W 2): T 128, U 2     ascii m 100 (W 4): T  64, U 1


def seam_id(run):
    (profile, P, m, W), rc = run
    return f"{profile}-m{m}-T{lv.seam_T(P, W)}-U{lv.seam_U(P, W)}-{'rc' if rc else 'fwd'}"


def seams_hold_records(want, S, T, n_records):
    present = lv.seam_records_present(want, S)
    missing = [r for r in lv.seam_records(T, n_records) if r not in present]
    assert not missing, ("no expected record at target records", missing)


@pytest.mark.parametrize("run", SEAM_RUNS, ids=seam_id)
def test_staged_tile_seams_two_sets(sassy, run):
    """one chunk, more than 2 T + 9 target records: the walk stages three tiles; records T - 1, T, T + 1, 2 T - 1, 2 T and
    the last one are near-copies"""
    (profile, P, m, W), rc = run
    a, b, n_records = lv.seam_case(profile, P, m, W, rc, False)
    S, T = 2 if rc else 1, lv.seam_T(P, W)
    assert len(a) <= 300 and n_records == S * len(b) > 2 * T + 9
    want = pref.expected_pairs(profile, a, b, lv.SEAM_K, rc)
    seams_hold_records(want, S, T, n_records)
    s = sassy.Searcher(profile, rc=rc)
    s.set_option("pairs_chunks", 1)
    check_pairs(s.hamming_pairs(a, b, lv.SEAM_K), want)
    check_nearest(s.hamming_nearest(a, b, lv.SEAM_K), pref.nearest_of_pairs(want, len(a)))


@pytest.mark.parametrize("run", SEAM_RUNS, ids=seam_id)
def test_staged_tile_seams_self_mode(sassy, run):
    """the targets are the entries, so the list is as long as 2 T + 10 records need.  With one chunk a wavefront starts its
    walk at its strip's tile start (r_wave - rt = 0), inside the tile at a multiple of 64 S, or -- where T <= 192 S --
    behind a whole tile; a second run forces the chunk count of scan_levels.self_walk_chunks, under which some wavefront
    starts inside a tile at an offset that is no multiple of U (offsets are multiples of S: where U <= S, at one that is no
    multiple of 64 S).  The records do not depend on the chunk count."""
    (profile, P, m, W), rc = run
    a, _, n_records = lv.seam_case(profile, P, m, W, rc, True)
    S, T, U = 2 if rc else 1, lv.seam_T(P, W), lv.seam_U(P, W)
    assert n_records == S * len(a) > 2 * T + 9
    want, square = pref.expected_self(profile, a, lv.SEAM_K, rc)
    seams_hold_records(want, S, T, n_records)
    per_row = np.bincount(want["a_idx"], minlength=len(a))
    s = sassy.Searcher(profile, rc=rc)
    seen = set()
    for chunks in (1, lv.self_walk_chunks(len(a), S, T, U)):
        kinds = lv.self_walk_kinds(len(a), S, T, chunks)
        for kind, waves in kinds.items():  # some wavefront of every kind of start holds a record
            assert any(per_row[i0:i0 + 64].any() for i0 in waves), (chunks, kind)
        seen |= set(kinds)
        s.set_option("pairs_chunks", chunks)
        check_pairs(s.hamming_pairs(a, None, lv.SEAM_K), want)
        check_nearest(s.hamming_nearest(a, None, lv.SEAM_K), pref.nearest_of_pairs(square, len(a)))
    assert {"at", "inside"} <= seen and ("behind" in seen or T > 192 * S), sorted(seen)
