"""Searches in flight that share one text pass (switch shared_pass, c_abi.hip: the open group; filter_dna_kernel<.., G = 2>).
Every result must be record for record, cigars included, what the lone search_shard of the same pattern returns, and
the oracle's where the text is small enough to check on the host."""
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


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def mutate(rng, s, edits):
    s = bytearray(s)
    for _ in range(edits):
        t, p = rng.randrange(3), rng.randrange(len(s))
        if t == 0:
            s[p] = rng.choice(b"ACGT")
        elif t == 1:
            s.insert(p, rng.choice(b"ACGT"))
        elif len(s) > 1:
            del s[p]
    return bytes(s)


def searcher(sassy, shared, depth):
    s = sassy.Searcher("dna", rc=False)
    s.set_option("shared_pass", shared)
    s.set_pipe_depth(depth)
    return s


def _bench_text(sassy, n):
    buf = sassy.DeviceBuffer(n + 4096)
    sassy.generate_dna(buf.ptr, n, 42, 0)
    pats = []
    for j, seed in enumerate([43, 46, 47, 48]):
        p = bytes(oracle.generate_dna(seed, 0, 32).tobytes())
        pats.append(p)
        sassy.plant(buf.ptr, n, 0, n, 42 + j, p, 3, 1 << 20, phase=((1 << 20) // 5) * j // 64 * 64)
    return buf, pats


def _stream(s, pats, buf, n, depth, steps, k=3):
    out, pending = [], []
    for i in range(steps):
        pending.append((i % len(pats), s.search_shard_begin(pats[i % len(pats)], buf.ptr, 0, n, 0, n, k)))
        if len(pending) >= depth:
            j, t = pending.pop(0)
            out.append((j, canon(s.search_finish(t)), s.stats()))
    while pending:
        j, t = pending.pop(0)
        out.append((j, canon(s.search_finish(t)), s.stats()))
    return out


@pytest.mark.parametrize("n_mb", [64, 256])
def test_bench_shaped_streams_equal_lone_searches(sassy, n_mb):
    """The benchmark's shape: a resident random text with four patterns planted, |P| = 32, k = 3, a stream of searches
    rotating through the four patterns, 2 / 3 / 4 in flight, finished oldest first.  shared_pass 0 / 1 / 3 (3: every
    search waits for a partner) give the lone searches' records; with 3 the members report pass_patterns = 2."""
    n = n_mb << 20
    buf, pats = _bench_text(sassy, n)
    lone = searcher(sassy, 0, 1)
    want = [canon(lone.search_shard(p, buf.ptr, 0, n, 0, n, 3)) for p in pats]
    assert all(len(w[1]) >= n_mb // 2 for w in want)
    for shared in (0, 1, 3):
        for depth in (2, 3, 4):
            s = searcher(sassy, shared, depth)
            got = _stream(s, pats, buf, n, depth, 10)
            assert len(got) == 10
            for j, g, st in got:
                assert g == want[j], (shared, depth, j)
                assert st["fused"] == 1
                assert st["pass_patterns"] == (2 if shared == 3 else st["pass_patterns"])
                assert st["pass_patterns"] in (1, 2)
            if shared == 0:
                assert all(st["pass_patterns"] == 1 for _, _, st in got)
    # a slice small enough for the oracle: the same stream on its first 2 MiB
    m = 2 << 20
    host = oracle.generate_dna(42, 0, m).tobytes()
    s = searcher(sassy, 3, 3)
    small = sassy.DeviceBuffer(m + 256)
    small.upload(host)
    for j, g, st in _stream(s, pats, small, m, 3, 8):
        r = lone.search_shard(pats[j], small.ptr, 0, m, 0, m, 3)
        assert g == canon(r)
        assert [key(x) for x in r.matches] == [key(x) for x in oracle.search("dna", pats[j], host, 3)]
    small.free()
    buf.free()


def test_mixed_tickets_around_an_open_group(sassy):
    """Groupable tickets interleaved with tickets that cannot join (other k with the paired filter, a second buffer, a
    halo shard, other flags), finished newest first and oldest first, one discarded with a NULL result pointer,
    ALL_MINIMA and WITHOUT_TRACE tickets, and a searcher freed with a ticket waiting in its open group."""
    rng = random.Random(11)
    n = (1 << 22) + 640
    pats = [rand_seq(rng, m) for m in (32, 32, 23, 32, 40, 24)]
    ks = [3, 3, 3, 2, 3, 1]
    text = bytearray(oracle.generate_dna(7, 0, n).tobytes())
    for p, k in zip(pats, ks):
        for _ in range(40):
            ins = mutate(rng, p, rng.randrange(0, k + 1))
            at = rng.randrange(0, n - 100)
            text[at:at + len(ins)] = ins
    text = bytes(text[:n])
    buf = sassy.DeviceBuffer(n + 256)
    buf.upload(text)
    buf2 = sassy.DeviceBuffer(n + 256)
    buf2.upload(text[::-1])
    lone = searcher(sassy, 0, 1)
    L = sassy.lib()
    for shared in (3, 1, 2):
        s = searcher(sassy, shared, 4)
        # (pattern, buffer, halo, shard_len, offset, k, flags)
        halo = sassy.required_halo(40, 3)
        a = 1 << 21
        jobs = [(0, buf, 0, n, 0, 3, 0), (2, buf, 0, n, 0, 3, 0), (1, buf, 0, n, 0, 3, 0), (3, buf2, 0, n, 0, 2, 0),
                (4, buf, halo, n - a, a, 3, 0), (5, buf, 0, n, 0, 1, 0), (0, buf, 0, n, 0, 3, sassy.ALL_MINIMA),
                (1, buf, 0, n, 0, 3, sassy.ALL_MINIMA), (3, buf, 0, n, 0, 2, sassy.WITHOUT_TRACE),
                (0, buf, 0, n, 0, 3, sassy.WITHOUT_TRACE), (4, buf, 0, a, 0, 3, 0), (1, buf, halo, n - a, a, 3, 0)]
        pending = []
        for i, (pi, b, h, sl, off, k, fl) in enumerate(jobs):
            ptr = b.ptr + off - h
            pending.append((pi, b, h, sl, off, k, fl, s.search_shard_begin(pats[pi], ptr, h, sl, off, n, k, fl)))
            if len(pending) == 4:
                order = pending.pop() if i % 2 else pending.pop(0)  # newest first, then oldest first
                pi, b, h, sl, off, k, fl, t = order
                want = lone.search_shard(pats[pi], b.ptr + off - h, h, sl, off, n, k, fl)
                if i == 7:
                    assert L.sassy_hip_search_finish(s._h, t, None) == 0
                    continue
                assert canon(s.search_finish(t)) == canon(want), (shared, i)
        for pi, b, h, sl, off, k, fl, t in pending[::-1]:
            want = lone.search_shard(pats[pi], b.ptr + off - h, h, sl, off, n, k, fl)
            assert canon(s.search_finish(t)) == canon(want), (shared, "drain")
        # one-at-a-time calls still work on the same searcher
        assert canon(s.search_shard(pats[0], buf.ptr, 0, n, 0, n, 3)) == canon(lone.search_shard(pats[0], buf.ptr, 0, n, 0, n, 3))
    # the oracle on the first pattern
    assert [key(x) for x in lone.search_shard(pats[0], buf.ptr, 0, n, 0, n, 3).matches] == \
        [key(x) for x in oracle.search("dna", pats[0], text, 3)]
    # freed with a ticket waiting in its open group (shared_pass 3: the first groupable ticket always waits)
    s2 = searcher(sassy, 3, 3)
    s2.search_shard_begin(pats[0], buf.ptr, 0, n, 0, n, 3)
    del s2
    s3 = searcher(sassy, 3, 3)
    t = s3.search_shard_begin(pats[1], buf.ptr, 0, n, 0, n, 3)
    assert canon(s3.search_finish(t)) == canon(lone.search_shard(pats[1], buf.ptr, 0, n, 0, n, 3))
    assert s3.stats()["pass_patterns"] == 1
    buf.free()
    buf2.free()


def test_one_member_falls_back_alone(sassy):
    """A member whose reports need the classic chain (a flat plateau of cost 1 over 40 000 columns) reruns alone; the
    other member of its pass keeps the grouped launch's records.  Both equal the oracle."""
    rng = random.Random(3)
    pat = rand_seq(rng, 32)
    flat = b"A" * 16 + b"C" + b"A" * 15
    t = bytearray(rand_seq(rng, 300_000))
    for at in range(1000, 250_000, 3000):
        ins = mutate(rng, pat, rng.randrange(4))
        t[at:at + len(ins)] = ins
    text = bytes(t[:300_000]) + b"G" * 5000 + b"A" * 40_000 + b"G" * 4936
    n = len(text)
    buf = sassy.DeviceBuffer(n + 256)
    buf.upload(text)
    for order in ((pat, flat), (flat, pat)):
        s = searcher(sassy, 3, 2)
        t1 = s.search_shard_begin(order[0], buf.ptr, 0, n, 0, n, 3)
        t2 = s.search_shard_begin(order[1], buf.ptr, 0, n, 0, n, 3)
        res = []
        for p, tk in zip(order, (t1, t2)):
            r = s.search_finish(tk)
            st = s.stats()
            assert st["pass_patterns"] == 2
            assert st["fused"] == (0 if p == flat else 1), (p == flat, st["fused"])
            assert [key(x) for x in r.matches] == [key(x) for x in oracle.search("dna", p, text, 3)], p == flat
            res.append(len(r.matches))
        assert min(res) > 0
    buf.free()
