"""The block-pair piece test of the grouped pass (filter_dna_kernel<Q, .., G = 2, SRC>; csrc/piece_pair_step.h) on the texts
of tests/helpers/piece_pair_texts.py: every slot of either member is the only intact piece of copies whose piece bytes
straddle the border in front of an even and of an odd block, and of copies that share a block pair with the other member's;
texts whose last pair is half a pair; halo shards whose first block is odd; a text that makes every wave end segments in
mid-stream.  Every ticket's records must be, cigars included, the lone shared_pass = 0, depth-1, plane_cache = 0
searcher's, which are the oracle's on the host copy; the stats say that the fused launch at the ticket's piece length
produced them and that tickets behind the first shared a launch."""
import os
import sys
import time

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pass_shapes as ps  # noqa: E402
import pass_streams as st  # noqa: E402
import piece_pair_texts as pt  # noqa: E402
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


def run_streams(sassy, ctx, jobs, want, grouped=True):
    """Streams of 6 and 7 searches that alternate two jobs (the 7-step stream begins with the second), three in flight,
    finished oldest first and newest first, shared_pass 4 and 1, plane_cache 1 and 0: the grouped launch runs from the
    text, from the text while it writes the planes, and on the planes.  grouped: the two jobs fit one launch."""
    for shared in (4, 1):
        for planes in (1, 0):
            for steps, order in ((6, jobs), (7, jobs[::-1])):
                for newest in (False, True):
                    c = ctx + (shared, planes, steps, newest)
                    s = searcher(sassy, shared, 3, planes)
                    got = st.stream(s, order, 3, steps, newest)
                    assert len(got) == steps
                    for i, job, r, stats in got:
                        assert st.canon(r) == want[job.j], (c, i, job.j, len(r.matches), stats)
                        assert stats["piece_len"] == ps.piece_len(len(job.pattern), job.k), (c, i, stats)
                        # (a ticket rerun on the classic chain would equal the oracle without the launch under test)
                        assert stats["fused"] == 1, (c, i, stats)
                        if shared == 4 and not newest and i >= 1:
                            assert stats["pass_patterns"] == (2 if grouped else 1), (c, i, stats)
                        if i == 0 or not planes:
                            assert stats["plane_launches"] == 0, (c, i, stats)
                        if planes and not newest and i >= 2 and grouped:
                            assert stats["plane_launches"] >= 1, (c, i, stats)


@pytest.mark.parametrize("row", pt.ROWS, ids=ps.row_id)
def test_both_kinds_of_border_and_the_half_pair(sassy, row):
    """The row's text, the text less its last 37 bytes, and the text less its last block -- an odd count of blocks, a copy
    ending in the last one."""
    t0 = time.perf_counter()
    T = pt.pair_text(row)
    for name, text in (("whole", T.text), ("odd cut", T.odd), ("odd blocks", T.odd_blocks)):
        n = len(text)
        buf = resident(sassy, text)
        jobs = [st.whole(j, T.pats[j], buf, n, T.ks[j]) for j in (0, 1)]
        want = lone_results(sassy, jobs, text)
        assert want[0] != want[1] and all(len(w[1]) >= 100 for w in want), name
        run_streams(sassy, (ps.row_id(row), name), jobs, want)
        buf.free()
    print(f"{ps.row_id(row)}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("row", pt.HALO_ROWS, ids=ps.row_id)
def test_halo_shards_whose_first_block_is_odd_or_even(sassy, row, parity):
    """The text as the shards [0, 16 KiB) and [16 KiB, n), the right one with a halo of required_halo and of 64 bytes more: the
    filter's first block is odd with one and even with the other, so a lane streams an odd count of blocks with one of
    them -- its last pair is half a pair -- and the pairs fall on the other borders.  Right-shard streams of both
    members, and streams that alternate the left and the right shard of one member (two plane keys).
    The right shard is longer than a workgroup: a grid of one has no halves, and its searches would not share a launch;
    Q = 12 comes as two patterns of one shape (piece_pair_texts.HALO_ROWS says why)."""
    t0 = time.perf_counter()
    T = pt.pair_text(row)
    text, n = T.text, len(T.text)
    a = 16384
    assert n - a > ps.WORKGROUP
    halo = max((sassy.required_halo(len(p), k) + 63) // 64 * 64 for p, k in zip(T.pats, T.ks)) + 64 * parity
    assert 0 < halo < a
    buf = resident(sassy, text)
    left = [st.Job(j, T.pats[j], buf.ptr, 0, a, 0, n, T.ks[j]) for j in (0, 1)]
    right = [st.Job(2 + j, T.pats[j], buf.ptr + a - halo, halo, n - a, a, n, T.ks[j]) for j in (0, 1)]
    want = lone_results(sassy, left + right)
    lone = searcher(sassy, 0, 1, planes=0)
    for j in (0, 1):  # the left shard's records followed by the right shard's: the whole text's
        merged = sassy.merge_shards([st.lone(lone, left[j]), st.lone(lone, right[j])], 1)
        assert [st.key(x) for x in merged.matches] == [st.key(x) for x in oracle.search("dna", T.pats[j], text, T.ks[j])], j
    assert all(len(w[1]) >= 100 for w in want[2:])
    run_streams(sassy, (ps.row_id(row), "right", parity), right, want)
    for j in (0, 1):  # (two texts: never one launch)
        run_streams(sassy, (ps.row_id(row), "left / right", parity, j), [left[j], right[j]], want, grouped=False)
    buf.free()
    print(f"{ps.row_id(row)} halo parity {parity}: {time.perf_counter() - t0:.2f} s")


def test_segments_end_in_mid_stream(sassy):
    """A copy of each of the bench's two patterns every 256 bytes over three workgroups: 128 windows per wave and member
    against a queue pressure of 64, so every wave ends segments between block pairs, runs the chunk DP and streams on
    from the saved halves -- from the text and on planes."""
    t0 = time.perf_counter()
    text, pats, ks = pt.dense_text(pt.ROWS[1])
    n = len(text)
    buf = resident(sassy, text)
    jobs = [st.whole(j, pats[j], buf, n, ks[j]) for j in (0, 1)]
    want = lone_results(sassy, jobs, text)
    assert all(len(w[1]) >= n // 256 - 1 for w in want)
    run_streams(sassy, ("dense",), jobs, want)
    buf.free()
    print(f"dense: {time.perf_counter() - t0:.2f} s")
