"""The shared text pass staggered in halves of the grid (switch shared_pass = 1 / 4; pass_planner.h, c_abi.hip:
run_pass_launch, ScanJob::enqueue_pass).  Every result must be record for record, cigars included, what the lone
search_shard of a shared_pass = 0, depth-1 searcher returns, and the oracle's on texts of at most 4 MiB."""
import random

import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    assert sassy_amd.device_count() > 0, "no HIP device: the GPU tests must not silently skip"
    return sassy_amd


def canon(r):
    a, pool = r.array, r.pool
    return a.tobytes(), tuple(bytes(pool[int(o):int(o) + int(l)]) for o, l in zip(a["cigar_off"], a["cigar_len"]))


def key(m):
    return (m.pattern_idx, m.text_start, m.text_end, m.pattern_start, m.pattern_end, m.cost, m.strand, m.cigar)


def searcher(sassy, shared, depth):
    s = sassy.Searcher("dna", rc=False)
    s.set_option("shared_pass", shared)
    s.set_pipe_depth(depth)
    return s


def planted(sassy, n, stride, seeds=(43, 46, 47, 48)):
    """n bytes of device-generated random text with the patterns planted every `stride` bytes, apart from each other"""
    buf = sassy.DeviceBuffer(n + 4096)
    sassy.generate_dna(buf.ptr, n, 42, 0)
    pats = []
    for j, seed in enumerate(seeds):
        p = bytes(oracle.generate_dna(seed, 0, 32).tobytes())
        pats.append(p)
        sassy.plant(buf.ptr, n, 0, n, 42 + j, p, 3, stride, phase=(stride // (len(seeds) + 1)) * j // 64 * 64)
    return buf, pats


def stream(s, pats, buf, n, depth, steps, newest_first=False, k=3):
    """steps searches rotating through pats, depth in flight: (step, pattern index, result, stats) in finishing order"""
    out, pending = [], []
    for i in range(steps):
        pending.append((i, i % len(pats), s.search_shard_begin(pats[i % len(pats)], buf.ptr, 0, n, 0, n, k)))
        if len(pending) >= depth:
            i_, j, t = pending.pop() if newest_first else pending.pop(0)
            out.append((i_, j, s.search_finish(t), s.stats()))
    while pending:
        i_, j, t = pending.pop() if newest_first else pending.pop(0)
        out.append((i_, j, s.search_finish(t), s.stats()))
    return out


def lone_results(sassy, pats, buf, n, host=None, k=3):
    lone = searcher(sassy, 0, 1)
    want = [lone.search_shard(p, buf.ptr, 0, n, 0, n, k) for p in pats]
    if host is not None:
        for p, w in zip(pats, want):
            assert [key(x) for x in w.matches] == [key(x) for x in oracle.search("dna", p, host, k)]
    return [canon(w) for w in want], want


def check_streams(sassy, pats, buf, n, want, depths=(2, 3, 4), steps_list=(9, 10)):
    for shared in (1, 4):
        for depth in depths:
            for steps in steps_list:
                for newest in (False, True):
                    s = searcher(sassy, shared, depth)
                    got = stream(s, pats, buf, n, depth, steps, newest)
                    assert len(got) == steps
                    for i, j, r, st in got:
                        assert canon(r) == want[j], (shared, depth, steps, newest, i)
                        assert st["pass_patterns"] in (1, 2)
                    if shared == 4 and not newest and st["grid"] >= 2:
                        # oldest first: ticket i's first half goes with i-1's second, its second with i+1's first
                        for i, j, r, st in got:
                            if 0 < i < steps - 1:
                                assert st["pass_patterns"] == 2 and st["fused"] == 1, (depth, steps, i, st)
                    # a synchronous search after the stream has drained
                    assert canon(s.search_shard(pats[0], buf.ptr, 0, n, 0, n, 3)) == want[0]


@pytest.mark.parametrize("n_mb", [64, 256])
def test_bench_shaped_streams_equal_lone_searches(sassy, n_mb):
    """The benchmark's shape (four planted 32-mers, k = 3, one plant per MiB) at depth 2 / 3 / 4, shared_pass 1 and 4,
    even and odd numbers of steps, finished oldest first and newest first."""
    n = n_mb << 20
    buf, pats = planted(sassy, n, 1 << 20)
    want, res = lone_results(sassy, pats, buf, n)
    assert all(len(w.matches) >= n_mb // 2 for w in res)
    check_streams(sassy, pats, buf, n, want)
    buf.free()


def test_small_texts_against_the_oracle(sassy):
    """Texts the oracle checks: 2 MiB + 777 and 4 MiB - 5 bytes (the second half ends in a partly empty workgroup or the
    grid has few workgroups), and one so small that the grid is a single workgroup (whole launches)."""
    for n, stride in (((2 << 20) + 777, 1 << 15), ((4 << 20) - 5, 1 << 14), (40_000, 1 << 11)):
        buf, pats = planted(sassy, n, stride)
        host = bytes(buf.download(n))
        want, res = lone_results(sassy, pats, buf, n, host)
        assert all(len(w.matches) >= n // stride // 2 for w in res)
        check_streams(sassy, pats, buf, n, want, depths=(2, 3), steps_list=(5, 6))
        if n == 40_000:
            assert searcher(sassy, 0, 1).search_shard(pats[0], buf.ptr, 0, n, 0, n, 3) is not None
            s = searcher(sassy, 4, 2)
            t = s.search_shard_begin(pats[0], buf.ptr, 0, n, 0, n, 3)
            s.search_finish(t)
            assert s.stats()["grid"] == 1
        buf.free()


def test_partial_last_workgroup_of_the_second_half(sassy):
    """96 MiB + 12345 bytes: the lane chunks leave the grid's last workgroup (the end of H1) partly empty."""
    n = (96 << 20) + 12345
    buf, pats = planted(sassy, n, 1 << 15, seeds=(43, 46))
    want, res = lone_results(sassy, pats, buf, n)
    s = searcher(sassy, 4, 2)
    got = stream(s, pats, buf, n, 2, 6)
    blocks, bpl = (n + 63) // 64, got[0][3]["blocks_per_chunk"]
    chunks = (blocks + bpl - 1) // bpl
    assert chunks % 256 != 0 and blocks % bpl != 0, (n, bpl)
    check_streams(sassy, pats, buf, n, want, depths=(2, 3), steps_list=(5, 6))
    buf.free()


def test_dense_plants_press_in_both_halves(sassy):
    """Plants every 256 bytes: every wave's chunk queues press mid-stream, in the waves of both halves."""
    for n in ((32 << 20) + 999, (2 << 20) + 333):
        buf, pats = planted(sassy, n, 256, seeds=(43, 46))
        host = bytes(buf.download(n)) if n < (4 << 20) else None
        want, res = lone_results(sassy, pats, buf, n, host)
        assert all(len(w.matches) >= n // 256 // 2 for w in res)
        for shared in (1, 4):
            s = searcher(sassy, shared, 3)
            for i, j, r, st in stream(s, pats, buf, n, 3, 5):
                assert canon(r) == want[j], (shared, i)
                assert st["fused"] == 1
        buf.free()


def test_flat_plateau_member_as_either_partner(sassy):
    """The member of test_one_member_falls_back_alone (a flat plateau of cost 1 over 40 000 columns needs the classic
    chain) as the partner of a ticket's first half and of its second half: it reruns alone, its partners keep their
    records."""
    rng = random.Random(3)
    pat = bytes(rng.choice(b"ACGT") for _ in range(32))
    flat = b"A" * 16 + b"C" + b"A" * 15
    t = bytearray(rng.choice(b"ACGT") for _ in range(300_000))
    for at in range(1000, 250_000, 3000):
        ins = bytearray(pat)
        for _ in range(rng.randrange(4)):
            ins[rng.randrange(32)] = rng.choice(b"ACGT")
        t[at:at + 32] = ins
    text = bytes(t[:300_000]) + b"G" * 5000 + b"A" * 40_000 + b"G" * 4936
    n = len(text)
    buf = sassy.DeviceBuffer(n + 256)
    buf.upload(text)
    want = {p: [key(x) for x in oracle.search("dna", p, text, 3)] for p in (pat, flat)}
    assert len(want[pat]) >= 80
    # (pat, flat, pat): flat shares pat's second half and the next pat's first; (flat, pat, flat): the other way round
    for order in ((pat, flat, pat), (flat, pat, flat)):
        s = searcher(sassy, 4, 3)
        tickets = [s.search_shard_begin(p, buf.ptr, 0, n, 0, n, 3) for p in order]
        for i, (p, tk) in enumerate(zip(order, tickets)):
            r = s.search_finish(tk)
            st = s.stats()
            assert st["pass_patterns"] == 2
            assert st["fused"] == (0 if p == flat else 1), (i, p == flat, st["fused"])
            assert [key(x) for x in r.matches] == want[p], (i, p == flat)
    buf.free()


def test_tickets_that_cannot_join_and_odd_ends(sassy):
    """A ticket that cannot join (another buffer, the paired filter's shape, a halo shard, ALL_MINIMA) begun while a
    ticket holds its second half back; finish(t, NULL); a searcher freed with a half outstanding; a synchronous search
    after the stream has drained."""
    n = (1 << 22) + 640
    buf, pats = planted(sassy, n, 1 << 14)
    host = bytes(buf.download(n))
    buf2 = sassy.DeviceBuffer(n + 256)
    buf2.upload(host[::-1])
    rng = random.Random(12)
    p23 = bytes(rng.choice(b"ACGT") for _ in range(23))
    lone = searcher(sassy, 0, 1)
    L = sassy.lib()
    halo = sassy.required_halo(32, 3)
    a = 1 << 21
    # (pattern, buffer, halo, shard_len, offset, k, flags)
    odd = [(pats[1], buf2, 0, n, 0, 3, 0), (p23, buf, 0, n, 0, 3, 0), (pats[1], buf, halo, n - a, a, 3, 0),
           (pats[1], buf, 0, n, 0, 3, sassy.ALL_MINIMA)]
    assert [key(x) for x in lone.search_shard(pats[0], buf.ptr, 0, n, 0, n, 3).matches] == \
        [key(x) for x in oracle.search("dna", pats[0], host, 3)]
    for shared in (4, 1):
        for p, b, h, sl, off, k, fl in odd:
            for newest in (False, True):
                s = searcher(sassy, shared, 3)
                t0 = s.search_shard_begin(pats[0], buf.ptr, 0, n, 0, n, 3)  # (4: keeps its second half back)
                t1 = s.search_shard_begin(p, b.ptr + off - h, h, sl, off, n, k, fl)
                t2 = s.search_shard_begin(pats[2], buf.ptr, 0, n, 0, n, 3)
                jobs = [(pats[0], buf, 0, n, 0, 3, 0, t0), (p, b, h, sl, off, k, fl, t1), (pats[2], buf, 0, n, 0, 3, 0, t2)]
                for p_, b_, h_, sl_, off_, k_, fl_, t in (jobs[::-1] if newest else jobs):
                    w = lone.search_shard(p_, b_.ptr + off_ - h_, h_, sl_, off_, n, k_, fl_)
                    assert canon(s.search_finish(t)) == canon(w), (shared, fl, newest)
                assert canon(s.search_shard(pats[3], buf.ptr, 0, n, 0, n, 3)) == canon(lone.search_shard(pats[3], buf.ptr, 0, n, 0, n, 3))
    # finish(t, NULL) of a ticket that still needs a half, then its successor
    s = searcher(sassy, 4, 2)
    t0 = s.search_shard_begin(pats[0], buf.ptr, 0, n, 0, n, 3)
    assert L.sassy_hip_search_finish(s._h, t0, None) == 0
    t1 = s.search_shard_begin(pats[1], buf.ptr, 0, n, 0, n, 3)
    t2 = s.search_shard_begin(pats[2], buf.ptr, 0, n, 0, n, 3)
    assert L.sassy_hip_search_finish(s._h, t1, None) == 0
    assert canon(s.search_finish(t2)) == canon(lone.search_shard(pats[2], buf.ptr, 0, n, 0, n, 3))
    # freed with a half outstanding
    s2 = searcher(sassy, 4, 3)
    s2.search_shard_begin(pats[0], buf.ptr, 0, n, 0, n, 3)
    s2.search_shard_begin(pats[1], buf.ptr, 0, n, 0, n, 3)
    del s2
    s3 = searcher(sassy, 4, 3)
    t = s3.search_shard_begin(pats[1], buf.ptr, 0, n, 0, n, 3)
    assert canon(s3.search_finish(t)) == canon(lone.search_shard(pats[1], buf.ptr, 0, n, 0, n, 3))
    assert s3.stats()["pass_patterns"] == 1
    buf.free()
    buf2.free()
