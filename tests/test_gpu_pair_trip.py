"""The pair trip of the grouped pass (filter_dna_kernel<Q, .., G = 2, SRC>: one block pair per loop trip, the plane reader's
two register sets taking turns) on small texts: lanes that own 1 .. 5 blocks, an odd and an even count of iterations,
occurrences in the half pair an odd count cuts off and at both ends of the buffer, dense texts whose segments end at pair
ends, multi-word patterns and halo shards whose first owned column clamps a run.

A lane's loop count is the launch's, blocks per lane chunk + the blocks in front (>= 9, odd or even with the parity of the
shard's first block), whatever the lane owns: the short lanes here are the last ones of a text, which own fewer blocks
than the plane loads run ahead, as many, and one more -- behind them the trips go on over blocks nobody owns.

shared_pass = 4 staggers the launches in halves without timing, so the two-member launches from the text, writing planes and
reading planes are all reached: every ticket's records are the lone shared_pass = 0, depth-1, plane_cache = 0 searcher's
(the oracle's, on whole texts), every ticket reports fused = 1, and from the third ticket on plane_launches >= 1."""
import os
import random
import sys
import time

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import filter_adversary as fa  # noqa: E402
import pass_shapes as ps  # noqa: E402
import pass_streams as st  # noqa: E402
import piece_pair_texts as pt  # noqa: E402
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCK = fa.BLOCK
CHUNK = 8            # blocks per lane chunk of a text this short (stats: blocks_per_chunk)
SHARD_AT = 16384     # where the right shard of a halo test begins: a multiple of a lane chunk


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
    lone = searcher(sassy, 0, 1, planes=0)
    want = []
    for job in jobs:
        r = st.lone(lone, job)
        stats = lone.stats()
        assert stats["plane_launches"] == 0 and stats["pass_patterns"] == 1 and stats["fused"] == 1, (job.j, stats)
        if text is not None:
            assert [st.key(x) for x in r.matches] == [st.key(x) for x in oracle.search("dna", job.pattern, text, job.k)], job.j
        want.append(st.canon(r))
    return want


def run_streams(sassy, ctx, jobs, want, chunk=None):
    """Streams of 6 and 7 searches that alternate the two jobs (the 7-step stream begins with the second: either is member
    0), three in flight, finished oldest first, shared_pass = 4 with kept planes."""
    for steps, order in ((6, jobs), (7, jobs[::-1])):
        s = searcher(sassy, 4, 3)
        got = st.stream(s, order, 3, steps)
        assert len(got) == steps
        for i, job, r, stats in got:
            c = ctx + (steps, i, job.j)
            assert st.canon(r) == want[job.j], (c, len(r.matches), len(want[job.j][1]), stats)
            assert stats["fused"] == 1, (c, stats)
            if chunk is not None:
                assert stats["blocks_per_chunk"] == chunk, (c, stats)
            if i >= 1:
                assert stats["pass_patterns"] == 2, (c, stats)
            if i == 0:
                assert stats["plane_launches"] == 0, (c, stats)
            if i >= 2:
                assert stats["plane_launches"] >= 1, (c, stats)


def right_shard(sassy, buf, n, pats, ks, parity):
    """The jobs of the shard [SHARD_AT, n) with a halo of required_halo, whole blocks, and 64 bytes more with parity 1: the
    filter's first block is odd with one and even with the other, and with it the count of a lane's iterations."""
    halo = max((sassy.required_halo(len(p), k) + 63) // 64 * 64 for p, k in zip(pats, ks)) + 64 * parity
    assert 0 < halo < SHARD_AT and n - SHARD_AT > ps.WORKGROUP
    return [st.Job(j, pats[j], buf.ptr + SHARD_AT - halo, halo, n - SHARD_AT, SHARD_AT, n, ks[j]) for j in (0, 1)]


def bench_pair():
    row = pt.ROWS[1]
    assert (row.q, row.a.m, row.b.m) == (8, 32, 32)
    return [ps.pattern(row.a), ps.pattern(row.b)], [row.a.k, row.b.k]


def planted(n, pats, at, seed):
    """n bytes of filler with a pattern at every at[i] (apart), the two taking turns as 0 1 1 0: neighbours differ and
    so do the neighbours of neighbours"""
    text = bytearray(fa.filler(random.Random(seed), n))
    for i, a in enumerate(sorted(at)):
        p = pats[(i + i // 2) % 2]
        if 0 <= a and a + len(p) <= n:
            text[a:a + len(p)] = p
    return bytes(text)


def check_whole_and_shards(sassy, ctx, text, pats, ks, min_matches, chunk=None):
    n = len(text)
    buf = resident(sassy, text)
    jobs = [st.whole(j, pats[j], buf, n, ks[j]) for j in (0, 1)]
    want = lone_results(sassy, jobs, text)
    assert want[0] != want[1] and all(len(w[1]) >= min_matches for w in want), (ctx, [len(w[1]) for w in want])
    run_streams(sassy, ctx + ("whole",), jobs, want, chunk)
    for parity in (0, 1):
        right = right_shard(sassy, buf, n, pats, ks, parity)
        want_r = lone_results(sassy, right)
        assert all(len(w[1]) >= min_matches // 2 for w in want_r), (ctx, parity)
        run_streams(sassy, ctx + ("right", parity), right, want_r, chunk)
    buf.free()


@pytest.mark.parametrize("tail", [1, 2, 3, 4, 5])
def test_short_last_lanes(sassy, tail):
    """Two workgroups, three whole lane chunks and a last lane that owns `tail` blocks (the shard [16 KiB, n) likewise: 16
    KiB are whole chunks) -- fewer blocks than the loads run ahead, as many, one more.  Every block of the last two lanes
    holds an occurrence of either member, the last block one that ends in the text's last column."""
    t0 = time.perf_counter()
    pats, ks = bench_pair()
    n_blocks = 2 * (ps.WORKGROUP // BLOCK) + 3 * CHUNK + tail
    n = n_blocks * BLOCK
    at = [b * BLOCK + 9 for b in range(n_blocks - tail - CHUNK, n_blocks - 1)] + [n - 32]
    at += list(range(1000, n - 2048, 3001))
    text = planted(n, pats, at, 40 + tail)
    check_whole_and_shards(sassy, ("tail", tail), text, pats, ks, 40, CHUNK)
    print(f"tail {tail}: {time.perf_counter() - t0:.2f} s")


def test_occurrences_at_the_ends_and_in_the_half_pair(sassy):
    """With an odd count of iterations a lane's last owned block is the first of a pair whose second is no iteration: an
    occurrence in the last block of every other lane chunk, and in its first.  A copy at byte 0 and one whose last
    byte is the buffer's (matches that end in the first m + k columns and in the last one), and copies around the shard's
    first byte: one that ends in its first owned block and one that straddles it (the run's first column is clamped)."""
    t0 = time.perf_counter()
    pats, ks = bench_pair()
    n_blocks = 2 * (ps.WORKGROUP // BLOCK) + 5 * CHUNK
    n = n_blocks * BLOCK
    at = [0, n - 32, n - 64 - 40]
    at += [SHARD_AT - 40, SHARD_AT + 40, SHARD_AT + 2 * BLOCK + 1]
    for lane_chunk in range(3, n_blocks // CHUNK, 2):
        if abs(lane_chunk * CHUNK * BLOCK - SHARD_AT) > 1024:
            at += [lane_chunk * CHUNK * BLOCK + 3, (lane_chunk + 1) * CHUNK * BLOCK - 34]  # its first block; ends in its last
    text = planted(n, pats, at, 50)
    check_whole_and_shards(sassy, ("ends",), text, pats, ks, 200, CHUNK)
    # the same with the last 37 bytes cut: the last block is not whole
    check_whole_and_shards(sassy, ("ends, odd cut",), text[:-ps.ODD_CUT], pats, ks, 200, CHUNK)
    print(f"ends: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("sparse", [None, 0, 1])
def test_dense_text_ends_segments_at_pair_ends(sassy, sparse):
    """A copy of each member every 256 bytes over three workgroups (128 windows per wave and member against a queue
    pressure of 64): every wave ends segments in mid-stream, at a pair's end, and goes on from the saved state.  sparse:
    that member keeps one copy in 64 -- only the other member's queue fills up, and both are saved and restored."""
    t0 = time.perf_counter()
    text, pats, ks = pt.dense_text(pt.ROWS[1])
    n = len(text)
    if sparse is not None:
        text = bytearray(text)
        fill = fa.filler(random.Random(12), n)
        for i, a in enumerate(range(128 * sparse, n - 256, 256)):
            if i % 64:
                text[a:a + 32] = fill[a:a + 32]
        text = bytes(text)
    buf = resident(sassy, text)
    jobs = [st.whole(j, pats[j], buf, n, ks[j]) for j in (0, 1)]
    want = lone_results(sassy, jobs, text)
    for j in (0, 1):
        assert len(want[j][1]) >= (n // 256 // 64 - 1 if j == sparse else n // 256 - 1), (sparse, j, len(want[j][1]))
    run_streams(sassy, ("dense", sparse), jobs, want)
    buf.free()
    print(f"dense, sparse member {sparse}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("row", [pt.HALO_ROWS[2], pt.HALO_ROWS[0]], ids=ps.row_id)
def test_multi_word_patterns_on_whole_texts_and_halo_shards(sassy, row):
    """Q = 12 as two patterns of 64 rows (two pattern words, 16 rows behind the last piece: the marks leave the block) and
    Q = 7 with 4 + 3 slots, on the sole-survivor text of tests/helpers/piece_pair_texts.py: the whole text, and its right
    shard with the filter's first block odd and even."""
    t0 = time.perf_counter()
    T = pt.pair_text(row)
    check_whole_and_shards(sassy, (ps.row_id(row),), T.text, T.pats, T.ks, 100)
    print(f"{ps.row_id(row)}: {time.perf_counter() - t0:.2f} s")


def test_eighty_rows_behind_the_last_piece(sassy):
    """(128, 3) with (36, 2): Q = 12, four pattern words, 80 rows behind member 0's last piece -- the columns of a hit lie a
    block and more behind the block that holds it."""
    t0 = time.perf_counter()
    row = next(r for r in ps.PAIRS if (r.a, r.b) == (ps.M(128, 3), ps.M(36, 2)))
    J = ps.row_text(row)
    for name, text in (("whole", J.text), ("odd cut", J.odd)):
        n = len(text)
        buf = resident(sassy, text)
        jobs = [st.whole(j, J.pats[j], buf, n, J.ks[j]) for j in (0, 1)]
        want = lone_results(sassy, jobs, text)
        assert all(len(w[1]) >= 500 for w in want)
        run_streams(sassy, (ps.row_id(row), name), jobs, want)
        buf.free()
    print(f"{ps.row_id(row)}: {time.perf_counter() - t0:.2f} s")
