"""The grouped text pass (filter_dna_kernel<.., G = 2>) at its own LDS size: the tile and two chunk queues per wave, no
pipelining pad, three workgroups per CU.  More waves share a CU than before, so each case below looks at a place where
waves of one pass differ: a partial last workgroup, queues that fill up mid-stream, and a member that needs the classic
chain.  Every result must equal the lone search_shard of the same pattern, cigars included, and the oracle where the text
is small enough to check on the host."""
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


def planted(sassy, n, stride, seeds=(43, 46)):
    """n bytes of device-generated random text with two patterns planted every `stride` bytes, apart from each other"""
    buf = sassy.DeviceBuffer(n + 4096)
    sassy.generate_dna(buf.ptr, n, 42, 0)
    pats = []
    for j, seed in enumerate(seeds):
        p = bytes(oracle.generate_dna(seed, 0, 32).tobytes())
        pats.append(p)
        sassy.plant(buf.ptr, n, 0, n, 42 + j, p, 3, stride, phase=(stride // 2) * j // 64 * 64)
    return buf, pats


def grouped_stream(s, pats, buf, n, steps, k=3):
    """steps searches rotating through pats, two in flight, finished oldest first: (pattern index, result, stats)"""
    out, pending = [], []
    for i in range(steps):
        pending.append((i % len(pats), s.search_shard_begin(pats[i % len(pats)], buf.ptr, 0, n, 0, n, k)))
        if len(pending) == 2:
            j, t = pending.pop(0)
            out.append((j, s.search_finish(t), s.stats()))
    while pending:
        j, t = pending.pop(0)
        out.append((j, s.search_finish(t), s.stats()))
    return out


def check_against_lone(sassy, pats, buf, n, steps, oracle_text=None):
    lone = searcher(sassy, 0, 1)
    want = [lone.search_shard(p, buf.ptr, 0, n, 0, n, 3) for p in pats]
    if oracle_text is not None:
        for p, w in zip(pats, want):
            assert [key(x) for x in w.matches] == [key(x) for x in oracle.search("dna", p, oracle_text, 3)]
    s = searcher(sassy, 3, 2)  # (3: every groupable search waits for a partner)
    got = grouped_stream(s, pats, buf, n, steps)
    assert len(got) == steps
    for j, r, st in got:
        assert st["pass_patterns"] == 2
        assert canon(r) == canon(want[j]), j
    return want, got


def test_partial_last_workgroup(sassy):
    """Text sizes whose lane chunks leave the grid's last workgroup partly empty (and its last lane's chunk short)."""
    for n in ((96 << 20) + 12345, (2 << 20) + 777):
        buf, pats = planted(sassy, n, 1 << 15)
        host = None
        if n < (4 << 20):
            host = bytes(buf.download(n))
        want, got = check_against_lone(sassy, pats, buf, n, 6, host)
        blocks, bpl = (n + 63) // 64, got[0][2]["blocks_per_chunk"]
        chunks = (blocks + bpl - 1) // bpl
        assert chunks % 256 != 0 and blocks % bpl != 0, (n, bpl)
        assert all(len(w.matches) >= n // (1 << 15) // 2 for w in want)
        buf.free()


def test_dense_plants_press_mid_stream(sassy):
    """Both members' patterns every 256 bytes: a wave queues ~128 chunks per member over its lane chunks, twice the press
    point of its queue, so every wave runs chunk-DP segments for both members in the middle of its stream."""
    for n in ((32 << 20) + 999, (2 << 20) + 333):
        buf, pats = planted(sassy, n, 256)
        host = bytes(buf.download(n)) if n < (4 << 20) else None
        want, got = check_against_lone(sassy, pats, buf, n, 4, host)
        assert all(st["fused"] == 1 for _, _, st in got)
        assert all(len(w.matches) >= n // 256 // 2 for w in want)
        buf.free()


def test_member_falls_back_beside_a_dense_partner(sassy):
    """One member needs the classic chain (a flat plateau of cost 1 over 40 000 columns) and reruns alone; its partner
    has a planted pattern every 512 bytes and keeps the grouped launch's records.  Both orders; both equal the lone
    searches and the oracle."""
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
    lone = searcher(sassy, 0, 1)
    for order in ((pat, flat), (flat, pat)):
        s = searcher(sassy, 3, 2)
        tickets = [s.search_shard_begin(p, buf.ptr, 0, n, 0, n, 3) for p in order]
        for p, tk in zip(order, tickets):
            r = s.search_finish(tk)
            st = s.stats()
            assert st["pass_patterns"] == 2
            assert st["fused"] == (0 if p == flat else 1)
            assert canon(r) == canon(lone.search_shard(p, buf.ptr, 0, n, 0, n, 3)), p == flat
            assert [key(x) for x in r.matches] == [key(x) for x in oracle.search("dna", p, text, 3)], p == flat
            assert len(r.matches) > (0 if p == flat else 1000)
    buf.free()
