"""The grouped and kept-plane text passes (filter_dna_kernel<Q, .., G, SRC>; launch_filter_group, launch_filter_kept,
ScanJob::enqueue_pass, c_abi.hip: run_pass_launch) at every piece length Q = 7 .. 12, with members of unequal piece
counts, rows behind the last piece, lone shapes of 7 and 8 pieces, planes written at one piece length and read at
another, and halo shards of both parities of the filter's first block -- on the adversarial texts of
tests/helpers/pass_shapes.py, where a copy's only intact piece is one named slot.  Every result must be record for record,
cigars included, what the lone search_shard of a shared_pass = 0, depth-1, plane_cache = 0 searcher returns, and the
oracle's on the host copy of the text.  The stats say that the launch under test produced it: piece_len, fused,
pass_patterns, plane_launches."""
import os
import sys
import time

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pass_shapes as ps  # noqa: E402
import pass_streams as st  # noqa: E402
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    assert sassy_amd.device_count() > 0, "no HIP device: the GPU tests must not silently skip"
    return sassy_amd


def searcher(sassy, shared, depth, planes=1):
    s = sassy.Searcher("dna", rc=False)
    s.set_option("shared_pass", shared)
    s.set_option("plane_cache", planes)
    s.set_pipe_depth(depth)
    return s


def resident(sassy, text):
    buf = sassy.DeviceBuffer(len(text) + 4096)
    buf.upload(text)
    return buf


def lone_results(sassy, jobs, text=None):
    """canon of every job's lone search; text: the host copy, whose oracle records the lone searches of whole texts equal"""
    lone = searcher(sassy, 0, 1, planes=0)
    want = []
    for job in jobs:
        r = st.lone(lone, job)
        stats = lone.stats()
        assert stats["plane_launches"] == 0 and stats["pass_patterns"] == 1
        assert stats["piece_len"] == ps.piece_len(len(job.pattern), job.k), (job.j, stats)
        if text is not None:
            assert [st.key(x) for x in r.matches] == [st.key(x) for x in oracle.search("dna", job.pattern, text, job.k)], job.j
        want.append(st.canon(r))
    return want


def check_ticket(ctx, i, job, r, stats, want):
    """What every ticket of every stream here owes: the lone search's records, from the fused launch at its piece length"""
    assert st.canon(r) == want[job.j], (ctx, i, job.j, len(r.matches), stats)
    assert stats["piece_len"] == ps.piece_len(len(job.pattern), job.k), (ctx, i, stats)
    # (a ticket rerun on the classic chain would equal the oracle without the launch under test having produced anything)
    assert stats["fused"] == 1, (ctx, i, stats)


@pytest.mark.parametrize("row", ps.PAIRS, ids=ps.row_id)
def test_every_piece_length_grouped_and_kept(sassy, row):
    """Streams of 6 and 7 searches that alternate the row's two patterns (the 7-step stream begins with the second, so
    either is member 0 of a grouped launch and either meets the first, writing launch), three in flight, finished oldest
    first and newest first, shared_pass 4 and 1, plane_cache 1 and 0, on the pair's text and on the text less its last 37
    bytes.  shared_pass = 4, oldest first: begin(i) launches one half for tickets i-1 and i together (a pair: the grouped
    launch at Q, raw or on planes), or -- two lone shapes never fit -- ticket i-1's second half and ticket i's first, each
    alone; the first ticket's halves write the planes and every later launch reads them."""
    t0 = time.perf_counter()
    J = ps.row_text(row)
    for text in (J.text, J.odd):
        n = len(text)
        buf = resident(sassy, text)
        jobs = [st.whole(j, J.pats[j], buf, n, J.ks[j]) for j in (0, 1)]
        want = lone_results(sassy, jobs, text)
        assert want[0] != want[1] and len(want[0][1]) >= 500
        for shared in (4, 1):
            for planes in (1, 0):
                for steps, order in ((6, jobs), (7, jobs[::-1])):
                    for newest in (False, True):
                        ctx = (ps.row_id(row), n, shared, planes, steps, newest)
                        s = searcher(sassy, shared, 3, planes)
                        got = st.stream(s, order, 3, steps, newest)
                        assert len(got) == steps
                        for i, job, r, stats in got:
                            check_ticket(ctx, i, job, r, stats, want)
                            assert (stats["grid"], stats["blocks_per_chunk"]) == (ps.grid_of(n)[0], 8), (ctx, i, stats)
                            if i == 0 or not planes:
                                assert stats["plane_launches"] == 0, (ctx, i, stats)
                            if shared == 4 and not newest and i >= 1:
                                assert stats["pass_patterns"] == (1 if row.lone else 2), (ctx, i, stats)
                            if row.lone:
                                assert stats["pass_patterns"] == 1, (ctx, i, stats)
                            if planes and not newest and i >= 2:
                                assert stats["plane_launches"] >= 1, (ctx, i, stats)
        buf.free()
    print(f"{ps.row_id(row)}: {time.perf_counter() - t0:.2f} s")


def test_planes_written_at_one_piece_length_read_at_another(sassy):
    """PlaneKey holds the text and the launch geometry, and no m, k or piece length: on a whole text the geometry does not
    depend on the pattern, so four tickets of Q = 7, 8, 10, 12 -- no two of which fit one launch -- use one store, written
    by the first ticket's launches at Q = 7 and read by every launch behind them.  Then (32, 3) gives its place to a second
    (40, 3) pattern: two Q = 10 tickets that may share launches among tickets that fit nobody."""
    t0 = time.perf_counter()
    J = ps.mixed_text(ps.MIXED)
    twin = ps.mixed_text([ps.MIXED[0], ps.MIXED_TWIN, ps.MIXED[2], ps.MIXED[3]], ps.MIXED)
    n = len(J.text)
    assert n < (1 << 20) and sorted(ps.piece_len(len(p), k) for p, k in zip(J.pats, J.ks)) == [7, 8, 10, 12]
    buf = resident(sassy, J.text)
    for T, mixed in ((J, True), (twin, False)):
        jobs = [st.whole(j, T.pats[j], buf, n, T.ks[j]) for j in range(4)]
        want = lone_results(sassy, jobs, J.text)
        # (every pattern whose layout the text holds; the twin's copies are none of the text's)
        assert len(set(want)) == 4 and all(len(w[1]) >= 500 for j, w in enumerate(want) if mixed or j != 1)
        for shared in (4, 1):
            for newest in (False, True):
                ctx = ("mixed" if mixed else "twin", shared, newest)
                s = searcher(sassy, shared, 4)
                got = st.stream(s, jobs, 4, 9, newest)
                assert len(got) == 9
                for i, job, r, stats in got:
                    check_ticket(ctx, i, job, r, stats, want)
                    if mixed:  # group_fits wants equal piece lengths
                        assert stats["pass_patterns"] == 1, (ctx, i, stats)
                    if i == 0:
                        assert stats["plane_launches"] == 0, (ctx, stats)
                    if not newest and i >= 2:
                        assert stats["plane_launches"] >= 1, (ctx, i, stats)
                assert sum(stats["plane_launches"] for _, _, _, stats in got) > 0, ctx
    buf.free()
    print(f"mixed: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("parity", [0, 1])
def test_kept_planes_on_halo_shards(sassy, parity):
    """The (32, 3) + (32, 3) text as the shards [0, a) and [a, n), the right one with a halo of required_halo(32, 3) and of
    64 bytes more: the filter's first block (first_owned less the blocks it looks back into) is odd with one and even with
    the other, so a lane's warm-up in front of its chunk is one block or two, and with it where the chunk's planes lie in
    the store.  A stream of right-shard searches keeps planes; a stream that alternates the left and the right shard has
    two keys, and neither shard's launch may read the other's planes -- the records decide."""
    t0 = time.perf_counter()
    row = next(r for r in ps.PAIRS if (r.a, r.b) == (ps.M(32, 3), ps.M(32, 3, 1)))
    J = ps.row_text(row)
    text, n = J.text, len(J.text)
    a = n // 2 // 64 * 64
    halo = (sassy.required_halo(32, 3) + 63) // 64 * 64 + 64 * parity
    assert 0 < halo < a
    buf = resident(sassy, text)
    left = [st.Job(j, J.pats[j], buf.ptr, 0, a, 0, n, 3) for j in (0, 1)]
    right = [st.Job(2 + j, J.pats[j], buf.ptr + a - halo, halo, n - a, a, n, 3) for j in (0, 1)]
    want = lone_results(sassy, left + right)
    lone = searcher(sassy, 0, 1, planes=0)
    for j in (0, 1):  # the left shard's records followed by the right shard's: the whole text's
        merged = sassy.merge_shards([st.lone(lone, left[j]), st.lone(lone, right[j])], 1)
        assert [st.key(x) for x in merged.matches] == [st.key(x) for x in oracle.search("dna", J.pats[j], text, 3)], j
    # (A's layout is the left half of the text and B's the right: each shard holds one pattern's copies)
    assert len(want[0][1]) >= 500 and len(want[3][1]) >= 500
    for shared in (4, 1):
        for steps, order in ((6, right), (7, right[::-1])):
            for newest in (False, True):
                ctx = (parity, halo, shared, steps, newest)
                s = searcher(sassy, shared, 3)
                got = st.stream(s, order, 3, steps, newest)
                for i, job, r, stats in got:
                    check_ticket(ctx + ("right",), i, job, r, stats, want)
                    if i == 0:
                        assert stats["plane_launches"] == 0, (ctx, stats)
                    if not newest and i >= 2:
                        assert stats["plane_launches"] >= 1, (ctx, i, stats)
                for j in (0, 1):
                    s = searcher(sassy, shared, 3)
                    for i, job, r, stats in st.stream(s, [left[j], right[j]], 3, steps, newest):
                        check_ticket(ctx + ("left / right", j), i, job, r, stats, want)
    buf.free()
    print(f"halo parity {parity}: {time.perf_counter() - t0:.2f} s")
