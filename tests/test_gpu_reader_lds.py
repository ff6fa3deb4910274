"""The plane-reading launches (filter_dna_kernel<Q, .., G, kPlaneRead>) at their own LDS layout (csrc/pass_lds.h): no
staging tile, the segment state right behind the chunk DP's carries and the chunk queues right behind the state, four
workgroups per CU.  Each case below puts work where that layout could go wrong: waves that save and restore their state
around a mid-stream chunk DP with both queues in use, the fullest DP area (four pattern words per member) next to the
state, the smallest and the largest piece-row table in front of the launch's LDS, a partial last workgroup, halo shards of
both parities of the first block, the one-member reader, and a member that leaves for the classic chain beside a dense
partner.

Streams run with shared_pass = 4, three searches in flight, finished oldest first: begin(i) launches one half of the grid
for tickets i-1 and i together, the first ticket's halves write the planes, and from the third ticket on every launch
reads them -- so those tickets must report plane_launches >= 1, pass_patterns == 2 (1: tickets that fit nobody) and, unless
they are meant to fall back, fused == 1.  Every ticket's records equal the lone search_shard's, cigars included, and the
oracle's on the host copy of the text (all texts here are below 4 MiB)."""
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, HERE)
import pass_shapes as ps  # noqa: E402
import pass_streams as st  # noqa: E402
from test_gpu_group_pass_lds import planted  # noqa: E402
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

DEPTH = 3


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


def plant_all(sassy, n, pats, stride, edits=3):
    """n bytes of device-generated random text with every pattern of pats planted every `stride` bytes, apart from each other"""
    buf = sassy.DeviceBuffer(n + 4096)
    sassy.generate_dna(buf.ptr, n, 42, 0)
    for j, p in enumerate(pats):
        sassy.plant(buf.ptr, n, 0, n, 42 + j, p, edits, stride, phase=(stride // 2) * j // 64 * 64)
    return buf


def lone_results(sassy, jobs, text=None):
    """canon of every job's lone search (no shared pass, no kept planes); text: the host copy the oracle searches"""
    lone = searcher(sassy, 0, 1, planes=0)
    want = []
    for job in jobs:
        r = st.lone(lone, job)
        stats = lone.stats()
        assert stats["plane_launches"] == 0 and stats["pass_patterns"] == 1, stats
        if text is not None:
            assert [st.key(x) for x in r.matches] == [st.key(x) for x in oracle.search("dna", job.pattern, text, job.k)], job.j
        want.append(st.canon(r))
    return want


def check_stream(sassy, ctx, jobs, want, steps, members=2, classic=()):
    """steps searches rotating through jobs at shared_pass 4, DEPTH in flight, oldest first; classic: the jobs (by j) that are
    meant to leave the fused launch"""
    s = searcher(sassy, 4, DEPTH)
    got = st.stream(s, jobs, DEPTH, steps)
    assert len(got) == steps and [i for i, _, _, _ in got] == list(range(steps))
    for i, job, r, stats in got:
        assert st.canon(r) == want[job.j], (ctx, i, job.j, len(r.matches), stats)
        assert stats["fused"] == (0 if job.j in classic else 1), (ctx, i, stats)
        if i == 0:
            assert stats["plane_launches"] == 0, (ctx, stats)
        if i >= 2:
            assert stats["plane_launches"] >= 1, (ctx, i, stats)
            assert stats["pass_patterns"] == members, (ctx, i, stats)
    return got


def whole_text_case(sassy, ctx, n, pats, stride, ks=None, steps=6, members=2, least=None):
    ks = ks or [3] * len(pats)
    buf = plant_all(sassy, n, pats, stride)
    text = bytes(buf.download(n))
    jobs = [st.whole(j, p, buf, n, k) for j, (p, k) in enumerate(zip(pats, ks))]
    want = lone_results(sassy, jobs, text)
    assert all(len(w[1]) >= (least if least is not None else n // stride // 2) for w in want), [len(w[1]) for w in want]
    got = check_stream(sassy, ctx, jobs, want, steps, members)
    for _, job, _, stats in got:
        assert stats["piece_len"] == ps.piece_len(len(job.pattern), job.k), (ctx, stats)
    buf.free()
    return got


def test_dense_plants_press_mid_stream_on_planes(sassy):
    """(a) Both members every 256 bytes: a wave queues about 128 chunks per member, twice its press point, so every wave of
    a reading launch saves its segment state, runs the chunk DP of both members and restores the state -- with the queues
    where the tile used to be."""
    n = (2 << 20) + 333
    buf, pats = planted(sassy, n, 256)
    text = bytes(buf.download(n))
    jobs = [st.whole(j, p, buf, n, 3) for j, p in enumerate(pats)]
    want = lone_results(sassy, jobs, text)
    assert all(len(w[1]) >= n // 256 // 2 for w in want)
    check_stream(sassy, "dense", jobs, want, 6)
    buf.free()


@pytest.mark.parametrize("q", [12, 7])
def test_fullest_dp_area_beside_the_state(sassy, q):
    """(b) Q = 12: two patterns of four words (|P| = 128, one of them tests/helpers/pass_shapes.py's), planted every 512
    bytes: the DP's four masks and 4 x 512 bytes of carries end exactly where the saved state begins -- carries that
    reached it would lose a run.  (c) Q = 7: the same with the smallest piece-row table in front of the launch's LDS."""
    if q == 12:
        pats = [bytes(oracle.generate_dna(43, 0, 128).tobytes()), ps.pattern(ps.M(128, 3))]
    else:
        pats = [ps.pattern(ps.M(29, 3)), bytes(oracle.generate_dna(46, 0, 30).tobytes())]
    assert all(ps.piece_len(len(p), 3) == q for p in pats)
    whole_text_case(sassy, ("dp area", q), (2 << 20) + 333, pats, 512)


def test_partial_last_workgroup_on_planes(sassy):
    """(d) A text whose lane chunks leave the grid's last workgroup partly empty and its last lane's chunk short."""
    n = (2 << 20) + 777
    pats = [bytes(oracle.generate_dna(seed, 0, 32).tobytes()) for seed in (43, 46)]
    got = whole_text_case(sassy, "partial", n, pats, 1 << 12)
    blocks, bpl = (n + 63) // 64, got[0][3]["blocks_per_chunk"]
    chunks = (blocks + bpl - 1) // bpl
    assert chunks % 256 != 0 and blocks % bpl != 0, (n, bpl)


@pytest.mark.parametrize("parity", [0, 1])
def test_halo_shards_of_both_parities_on_planes(sassy, parity):
    """(e) The right shard [a, n) with a halo of required_halo(32, 3) and of 64 bytes more: the filter's first block is odd
    with one and even with the other (n_iter is odd with one of them: a pair whose second block lies behind the last
    iteration), both members planted every 256 bytes."""
    n = (1 << 20) + 4321
    buf, pats = planted(sassy, n, 256)
    text = bytes(buf.download(n))
    a = n // 2 // 64 * 64
    halo = (sassy.required_halo(32, 3) + 63) // 64 * 64 + 64 * parity
    assert 0 < halo < a
    left = [st.Job(j, pats[j], buf.ptr, 0, a, 0, n, 3) for j in (0, 1)]
    right = [st.Job(2 + j, pats[j], buf.ptr + a - halo, halo, n - a, a, n, 3) for j in (0, 1)]
    want = lone_results(sassy, left + right)
    lone = searcher(sassy, 0, 1, planes=0)
    for j in (0, 1):  # the left shard's records followed by the right shard's: the whole text's
        merged = sassy.merge_shards([st.lone(lone, left[j]), st.lone(lone, right[j])], 1)
        assert [st.key(x) for x in merged.matches] == [st.key(x) for x in oracle.search("dna", pats[j], text, 3)], j
    assert all(len(want[2 + j][1]) >= (n - a) // 256 // 2 for j in (0, 1))
    for steps, order in ((6, right), (7, right[::-1])):
        check_stream(sassy, ("halo", parity, steps), order, want, steps)
    buf.free()


def test_one_member_reader(sassy):
    """(f) Two patterns of 8 pieces (|P| = 100, k = 7: Q = 12, four words) never fit one launch: every launch has one member,
    and from the second ticket's first half on every one reads planes -- at 7 440 bytes per wave instead of the padded
    tile's.  Planted every 256 bytes, so the lone reader too runs its chunk DP mid-stream beside the relocated state.  The
    stream's last ticket, and the second of a stream of two, has its second half held back while the pass before it
    streams, and gets it alone at its finish."""
    n = (2 << 20) + 333
    pats = [bytes(oracle.generate_dna(seed, 0, 100).tobytes()) for seed in (43, 46)]
    got = whole_text_case(sassy, "one member", n, pats, 256, ks=[7, 7], steps=5, members=1)
    assert all(stats["pass_patterns"] == 1 for _, _, _, stats in got)
    buf = plant_all(sassy, n, pats, 256)
    jobs = [st.whole(j, p, buf, n, 7) for j, p in enumerate(pats)]
    want = lone_results(sassy, jobs)
    s = searcher(sassy, 4, DEPTH)
    tickets = [st.begin(s, job) for job in jobs]
    for i, (job, t) in enumerate(zip(jobs, tickets)):
        r = s.search_finish(t)
        stats = s.stats()
        assert st.canon(r) == want[job.j], (i, stats)
        assert stats["fused"] == 1 and stats["pass_patterns"] == 1 and stats["plane_launches"] == (0 if i == 0 else 2), (i, stats)
    buf.free()


def test_member_falls_back_beside_a_dense_partner_on_planes(sassy):
    """(g) One member needs the classic chain (a flat plateau of cost 1 over 40 000 columns) and reruns alone; its partner
    has a planted pattern every 512 bytes and keeps the reading launch's records.  Three tickets, so that the third shares
    a reading half launch with the second: the flat pattern as either member of it."""
    rng = random.Random(5)
    pat = bytes(oracle.generate_dna(43, 0, 32).tobytes())
    flat = b"A" * 16 + b"C" + b"A" * 15
    n_rand = (1 << 20) + 4321
    t = bytearray(oracle.generate_dna(9, 0, n_rand).tobytes())
    for at in range(100, n_rand - 64, 512):
        s_ = bytearray(pat)
        for _ in range(rng.randrange(4)):
            s_[rng.randrange(32)] = rng.choice(b"ACGT")
        t[at:at + 32] = s_
    text = bytes(t) + b"G" * 5000 + b"A" * 40_000 + b"G" * 4937
    n = len(text)
    buf = sassy.DeviceBuffer(n + 256)
    buf.upload(text)
    jobs = [st.whole(0, pat, buf, n, 3), st.whole(1, flat, buf, n, 3)]
    want = lone_results(sassy, jobs, text)
    assert len(want[0][1]) > 1000
    for order in (jobs, jobs[::-1]):
        check_stream(sassy, ("fallback", order[0].j), order, want, 3, classic=(1,))
    buf.free()
