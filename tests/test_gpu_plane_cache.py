"""The text's code planes kept across a stream of searches in flight (switch plane_cache; plane_cache.h, c_abi.hip:
run_pass_launch, filter_dna_kernel<.., SRC>).  Every result must be record for record, cigars included, what the lone
search_shard of a shared_pass = 0, depth-1, plane_cache = 0 searcher returns, and the oracle's on texts of at most 4 MiB."""
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


def searcher(sassy, shared, depth, planes=1, cap_mb=0):
    s = sassy.Searcher("dna", rc=False)
    s.set_option("shared_pass", shared)
    s.set_option("plane_cache", planes)
    s.set_option("plane_cache_max_mb", cap_mb)
    s.set_pipe_depth(depth)
    return s


def planted(sassy, n, stride, seeds=(43, 46, 47, 48), text_seed=42):
    """n bytes of device-generated random text with the patterns planted every `stride` bytes, apart from each other"""
    buf = sassy.DeviceBuffer(n + 4096)
    sassy.generate_dna(buf.ptr, n, text_seed, 0)
    pats = []
    for j, seed in enumerate(seeds):
        p = bytes(oracle.generate_dna(seed, 0, 32).tobytes())
        pats.append(p)
        sassy.plant(buf.ptr, n, 0, n, text_seed + j, p, 3, stride, phase=(stride // (len(seeds) + 1)) * j // 64 * 64)
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
    lone = searcher(sassy, 0, 1, planes=0)
    want = [lone.search_shard(p, buf.ptr, 0, n, 0, n, k) for p in pats]
    assert lone.stats()["plane_launches"] == 0
    if host is not None:
        for p, w in zip(pats, want):
            assert [key(x) for x in w.matches] == [key(x) for x in oracle.search("dna", p, host, k)]
    return [canon(w) for w in want], want


def check_streams(sassy, pats, buf, n, want, depths=(2, 3, 4), steps_list=(5, 6), planes=1, cap_mb=0, kept=True):
    read = 0
    for shared in (1, 4):
        for depth in depths:
            for steps in steps_list:
                for newest in (False, True):
                    s = searcher(sassy, shared, depth, planes, cap_mb)
                    got = stream(s, pats, buf, n, depth, steps, newest)
                    assert len(got) == steps
                    for i, j, r, st in got:
                        assert canon(r) == want[j], (shared, depth, steps, newest, i)
                        if i == 0:  # the stream's first ticket finds nothing written
                            assert st["plane_launches"] == 0, (shared, depth, steps, newest, st)
                        if not kept:
                            assert st["plane_launches"] == 0, (shared, depth, steps, newest, i, st)
                        elif shared == 4 and not newest and i >= 2:
                            # oldest first: both halves are written by the first two begins, the third ticket reads
                            assert st["plane_launches"] >= 1 and st["fused"] == 1, (shared, depth, steps, i, st)
                        read += st["plane_launches"]
                    # a synchronous search after the stream has drained: the text, as ever
                    assert canon(s.search_shard(pats[0], buf.ptr, 0, n, 0, n, 3)) == want[0]
                    assert s.stats()["plane_launches"] == 0
    return read


@pytest.mark.parametrize("n,stride", [((2 << 20) + 777, 1 << 15), ((4 << 20) - 5, 1 << 14), (40_000, 1 << 11),
                                      ((96 << 20) + 12345, 1 << 15)])
def test_streams_on_kept_planes_equal_lone_searches(sassy, n, stride):
    """Depth 2 / 3 / 4, shared_pass 1 and 4, 5 and 6 steps, finished oldest first and newest first: a grid of a few
    workgroups whose second half ends partly empty, a grid of one workgroup (whole launches only), and 96 MiB + 12 345
    bytes (the grid's last workgroup partly empty)."""
    buf, pats = planted(sassy, n, stride)
    host = bytes(buf.download(n)) if n <= (4 << 20) else None
    want, res = lone_results(sassy, pats, buf, n, host)
    assert all(len(w.matches) >= n // stride // 2 for w in res)
    assert check_streams(sassy, pats, buf, n, want) > 0
    if n == 40_000:
        s = searcher(sassy, 4, 2)
        s.search_finish(s.search_shard_begin(pats[0], buf.ptr, 0, n, 0, n, 3))
        assert s.stats()["grid"] == 1
    buf.free()


def test_pressing_queues_resume_on_planes(sassy):
    """Plants every 256 bytes: every wave's chunk queues press mid-stream, so segments end and resume on planes."""
    n = (2 << 20) + 333
    buf, pats = planted(sassy, n, 256, seeds=(43, 46))
    host = bytes(buf.download(n))
    want, res = lone_results(sassy, pats, buf, n, host)
    assert all(len(w.matches) >= n // 256 // 2 for w in res)
    for shared in (1, 4):
        for depth in (3, 4):
            s = searcher(sassy, shared, depth)
            got = stream(s, pats, buf, n, depth, 6)
            for i, j, r, st in got:
                assert canon(r) == want[j], (shared, depth, i)
                assert st["fused"] == 1
            assert sum(st["plane_launches"] for _, _, _, st in got) >= 3, (shared, depth)
    buf.free()


def test_a_new_text_at_the_same_pointer_after_a_drain(sassy):
    """The safety case: a stream, drained; then another text uploaded to the same pointer and length and a second stream on
    the same searcher.  Its results are the new text's, and its first ticket reads no planes."""
    n = (4 << 20) - 5
    buf, pats = planted(sassy, n, 1 << 14)
    want_old, _ = lone_results(sassy, pats, buf, n)
    s = searcher(sassy, 4, 3)
    got = stream(s, pats, buf, n, 3, 6)
    assert all(canon(r) == want_old[j] for _, j, r, _ in got) and got[-1][3]["plane_launches"] >= 1
    # another text, other plants, the same pointer and length
    other, _ = planted(sassy, n, 1 << 14, text_seed=77)
    new_host = bytes(other.download(n))
    other.free()
    buf.upload(new_host)
    want_new, _ = lone_results(sassy, pats, buf, n, new_host)
    assert want_new != want_old
    got = stream(s, pats, buf, n, 3, 6)
    for i, j, r, st in got:
        assert canon(r) == want_new[j], i
        if i == 0:
            assert st["plane_launches"] == 0
        if i >= 2:
            assert st["plane_launches"] >= 1
    buf.free()


def test_a_foreign_ticket_among_open_ones(sassy):
    """Another buffer, a halo shard of the same buffer, m = 23 (the paired filter) and ALL_MINIMA, each begun while the
    planes of the stream's buffer are written and tickets are open: it reads no planes, its result is right, and so are
    its neighbours'."""
    n = (1 << 22) + 640
    buf, pats = planted(sassy, n, 1 << 14)
    host = bytes(buf.download(n))
    buf2 = sassy.DeviceBuffer(n + 256)
    buf2.upload(host[::-1])
    rng = random.Random(12)
    p23 = bytes(rng.choice(b"ACGT") for _ in range(23))
    lone = searcher(sassy, 0, 1, planes=0)
    halo = sassy.required_halo(32, 3)
    a = 1 << 21
    assert [key(x) for x in lone.search_shard(pats[0], buf.ptr, 0, n, 0, n, 3).matches] == \
        [key(x) for x in oracle.search("dna", pats[0], host, 3)]
    # (pattern, buffer, halo, shard_len, offset, k, flags)
    odd = [(pats[1], buf2, 0, n, 0, 3, 0), (p23, buf, 0, n, 0, 3, 0), (pats[1], buf, halo, n - a, a, 3, 0),
           (pats[1], buf, 0, n, 0, 3, sassy.ALL_MINIMA)]
    own = lambda p: (p, buf, 0, n, 0, 3, 0)
    for shared in (4, 1):
        for foreign in odd:
            for newest in (False, True):
                s = searcher(sassy, shared, 4)
                jobs = [own(pats[0]), own(pats[1]), foreign, own(pats[2])]
                tickets = [s.search_shard_begin(p, b.ptr + off - h, h, sl, off, n, k, fl) for p, b, h, sl, off, k, fl in jobs]
                order = list(range(4))[::-1] if newest else list(range(4))
                stats = {}
                for i in order:
                    p, b, h, sl, off, k, fl = jobs[i]
                    w = lone.search_shard(p, b.ptr + off - h, h, sl, off, n, k, fl)
                    assert canon(s.search_finish(tickets[i])) == canon(w), (shared, fl, newest, i)
                    stats[i] = s.stats()
                assert stats[0]["plane_launches"] == 0 and stats[2]["plane_launches"] == 0, (shared, newest, stats)
                assert stats[3]["plane_launches"] >= 1, (shared, newest, stats)  # (behind the foreign ticket: still kept)
    buf.free()
    buf2.free()


def test_flat_plateau_member_while_planes_are_in_use(sassy):
    """The member of test_flat_plateau_member_as_either_partner (a flat plateau of cost 1 over 40 000 columns needs the
    classic chain) as a partner in launches that write and that read planes: it reruns alone on the text, its partners keep
    their records."""
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
    for order in ((pat, pat, flat, pat), (flat, pat, flat, pat)):
        s = searcher(sassy, 4, 4)
        tickets = [s.search_shard_begin(p, buf.ptr, 0, n, 0, n, 3) for p in order]
        for i, (p, tk) in enumerate(zip(order, tickets)):
            r = s.search_finish(tk)
            st = s.stats()
            assert st["pass_patterns"] == 2
            assert st["fused"] == (0 if p == flat else 1), (i, p == flat, st["fused"])
            assert [key(x) for x in r.matches] == want[p], (i, p == flat)
            assert (st["plane_launches"] >= 1) == (i >= 1), (i, st)
    buf.free()


def test_cap_and_switch_give_the_parents_passes(sassy):
    """plane_cache_max_mb = 1 on the 4 MiB text (its store would be 1.25 MiB) and plane_cache = 0: the same records, and
    no launch reads planes."""
    n = (4 << 20) - 5
    buf, pats = planted(sassy, n, 1 << 14)
    want, _ = lone_results(sassy, pats, buf, n)
    assert check_streams(sassy, pats, buf, n, want, depths=(3,), cap_mb=1, kept=False) == 0
    assert check_streams(sassy, pats, buf, n, want, depths=(3,), planes=0, kept=False) == 0
    assert check_streams(sassy, pats, buf, n, want, depths=(3,), cap_mb=2) > 0  # (a cap the store fits under)
    buf.free()


def free_device_bytes(sassy):
    import ctypes as C
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert sassy.lib().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_serial_searches_make_no_store_and_keep_their_launch(sassy):
    """begin -> finish with nothing else in flight, at depth 1 and at depth 2 (shared_pass 1 and 0): no reader can follow,
    so no store is allocated (the device's free memory stays; an overlapping stream on the same text takes its 25 MiB),
    no launch reads planes, and the launch is the search's own -- the stats of a plane_cache = 0 searcher."""
    n = (96 << 20) + 12345
    buf, pats = planted(sassy, n, 1 << 15, seeds=(43, 46))
    want, _ = lone_results(sassy, pats, buf, n)
    same = ("grid", "fused", "piece_len", "pass_patterns", "plane_launches", "scan_launches", "blocks_per_chunk", "filtered")
    for depth, shared in ((1, 1), (2, 1), (2, 0)):
        ref = searcher(sassy, shared, depth, planes=0)
        ref.search_finish(ref.search_shard_begin(pats[0], buf.ptr, 0, n, 0, n, 3))
        ref_st = ref.stats()
        s = searcher(sassy, shared, depth)
        for j in (0, 1):  # (the lanes' own buffers are made here)
            assert canon(s.search_finish(s.search_shard_begin(pats[j], buf.ptr, 0, n, 0, n, 3))) == want[j]
        before = free_device_bytes(sassy)
        for i in range(4):
            r = s.search_finish(s.search_shard_begin(pats[i & 1], buf.ptr, 0, n, 0, n, 3))
            st = s.stats()
            assert canon(r) == want[i & 1]
            assert {f: st[f] for f in same} == {f: ref_st[f] for f in same}, (depth, shared, st)
            assert st["plane_launches"] == 0 and st["pass_patterns"] == 1
        assert before - free_device_bytes(sassy) < (8 << 20), (depth, shared)
        if depth == 2 and shared == 1:  # the same searcher, now with two in flight: the store appears
            got = stream(s, pats, buf, n, 2, 5)
            assert all(canon(r) == want[j] for _, j, r, _ in got) and got[-1][3]["plane_launches"] >= 1
            assert before - free_device_bytes(sassy) > (20 << 20)
    buf.free()
