"""GPU: the case-insensitive Ascii profile ("ascii_ci") against the folded oracle.

fold(x) = x.lower() on bytes folds exactly A-Z, and eq_ignore_ascii_case(a, b) <=> fold(a) == fold(b); so every result of
an ascii_ci search must equal the oracle's case-sensitive "ascii" search of fold(pattern) in fold(text), field by field
(the traceback's tie-breaks see only the match relation, so the cigars agree too)."""
import ctypes as C
import os
import random
import sys

import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import all_alignments_ref as aref  # noqa: E402
from helpers import best_matches_ref as bref  # noqa: E402
from helpers.prose_text import fold, on_device, prose  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    assert sassy_amd.device_count() > 0, "no HIP device: the GPU tests must not silently skip"
    return sassy_amd


def key(m):
    return (m.pattern_idx, m.text_start, m.text_end, m.pattern_start, m.pattern_end, m.cost, m.strand, m.cigar)


def same(got, want, ctx=None):
    g, w = [key(m) for m in got], [key(m) for m in want]
    assert g == w, (ctx, g[:4], w[:4], len(g), len(w))


def swap_case(rng, s, p=0.5):
    return bytes((c ^ 0x20) if (chr(c).isascii() and chr(c).isalpha() and rng.random() < p) else c for c in s)


def mutate(rng, s, edits):
    s = bytearray(s)
    for _ in range(edits):
        t, p = rng.randrange(3), rng.randrange(len(s))
        if t == 0:
            s[p] = rng.choice(b"abcXYZ_@[ \n\xe9")
        elif t == 1:
            s.insert(p, rng.choice(b"abcXYZ_@[ \n\xe9"))
        elif len(s) > 1:
            del s[p]
    return bytes(s)


def test_parity_across_shapes(sassy):
    """m = 1 .. 300 (64 and 65 included), k = 0 .. m/3, mixed-case prose with punctuation, digits, bytes >= 0x80, '_@[' and
    newlines; patterns cut from the text with their case swapped (cost 0 under the fold) and with edits; search,
    search_all and without_trace."""
    rng = random.Random(20261017)
    s = sassy.Searcher("ascii_ci", rc=False)
    text = prose(rng, 24_000)
    ft = fold(text)
    n_zero = 0
    for m in (1, 2, 3, 5, 8, 13, 20, 31, 32, 33, 47, 63, 64, 65, 66, 96, 127, 128, 129, 200, 300):
        ks = sorted({0, 1, m // 6, m // 3})
        for k in ks:
            if k > m // 3 and k > 0:
                continue
            at = rng.randrange(0, len(text) - m)
            pat = swap_case(rng, text[at:at + m])
            if k and m > 3:
                pat = mutate(rng, pat, rng.randrange(0, k + 1))
            if not pat:
                continue
            # texts of a size the oracle's naive DP takes quickly for long patterns
            t, f = (text, ft) if m <= 66 else (text[max(0, at - 3000):at + 3000], ft[max(0, at - 3000):at + 3000])
            want = oracle.search("ascii", fold(pat), f, k)
            got = s.search(pat, t, k)
            same(got, want, ("search", m, k))
            n_zero += sum(1 for x in got if x.cost == 0)
            if m >= 3:
                same(s.search_all(pat, t[:6000], k), oracle.search("ascii", fold(pat), f[:6000], k, all_minima=True), ("all", m, k))
            wt = s.search_without_trace(pat, t, k)
            assert [(x.text_end, x.cost) for x in wt] == [(x.text_end, x.cost) for x in want], ("without trace", m, k)
    assert n_zero >= 15


def test_byte_mode(sassy):
    """More than kMaxSlots = 64 distinct FOLDED bytes in the pattern: byte mode (the row table holds the folded bytes, the
    kernels fold the text's plane 5)."""
    rng = random.Random(7)
    s = sassy.Searcher("ascii_ci", rc=False)
    alphabet = bytes(range(33, 127)) + bytes(range(160, 256))
    for m, k in ((120, 0), (150, 6), (300, 20)):
        pat = bytes(rng.sample(alphabet, min(m, len(alphabet))))
        pat = (pat * 3)[:m]
        assert len(set(fold(pat))) > 64
        text = bytearray(prose(rng, 9000))
        for at, e in ((500, 0), (3000, k // 2), (6000, k)):
            ins = mutate(rng, swap_case(rng, pat), e)
            text[at:at + len(ins)] = ins
        text = bytes(text)
        want = oracle.search("ascii", fold(pat), fold(text), k)
        assert len(want) >= 2, (m, k)
        same(s.search(pat, text, k), want, ("bytes", m, k))
        same(s.search_all(pat, text, k), oracle.search("ascii", fold(pat), fold(text), k, all_minima=True), ("bytes all", m, k))


def test_discrimination_and_the_deviation(sassy):
    ci = sassy.Searcher("ascii_ci", rc=False)
    cs = sassy.Searcher("ascii", rc=False)
    text = b"status: Kernel TIMEOUT on Device 3\nstatus: ok\n"
    pat = b"kernel timeout"
    got = ci.search(pat, text, 0)
    assert [(m.text_start, m.text_end, m.cost, m.cigar) for m in got] == [(8, 22, 0, "14=")]
    assert cs.search(pat, text, 0) == []  # ascii is unchanged: case-sensitive, and ascii_ci is no alias of it
    same(cs.search(b"Kernel TIMEOUT", text, 0), oracle.search("ascii", b"Kernel TIMEOUT", text, 0))
    assert len(cs.search(b"Kernel TIMEOUT", text, 0)) == 1
    # is_match, not the reference's scan quirk: '_' (bit 5 clear, no letter) matches itself
    got = ci.search(b"a_b", b"xx A_B yy", 0)
    assert [(m.text_start, m.text_end, m.cost) for m in got] == [(3, 6, 0)]
    for c in b"_@[\n":
        p = bytes([c])
        assert [(m.text_start, m.cost) for m in ci.search(p, b"ab" + p + b"cd", 0)] == [(2, 0)], c
    # only letters fold: '@' (0x40) and '`' (0x60) differ in bit 5 alone, and so do '[' / '{' and 0xC9 / 0xE9
    for a, b in ((b"@", b"`"), (b"`", b"@"), (b"[", b"{"), (b"{", b"["), (b"\xc9", b"\xe9"), (b"\xe9", b"\xc9"), (b"\n", b"*")):
        assert ci.search(a, b"xx" + b + b"xx", 0) == [], (a, b)
    assert len(ci.search(b"z", b"--Z--", 0)) == 1 and len(ci.search(b"Z", b"--z--", 0)) == 1


def test_every_entry_point(sassy):
    rng = random.Random(99)
    ci = sassy.Searcher("ascii_ci", rc=False)
    text = prose(rng, 20_000)
    ft = fold(text)
    at = 7001
    pat = swap_case(rng, text[at:at + 24])
    k = 2
    want = oracle.search("ascii", fold(pat), ft, k)
    assert any(m.cost == 0 for m in want)
    buf, dev = on_device(sassy, text)
    # search / search_all / without_trace, host and device text
    same(ci.search(pat, text, k), want, "host")
    same(ci.search(pat, dev, k), want, "device")
    want_all = oracle.search("ascii", fold(pat), ft, k, all_minima=True)
    same(ci.search_all(pat, dev, k), want_all, "device all")
    assert [(m.text_end, m.cost) for m in ci.search_without_trace(pat, dev, k)] == [(m.text_end, m.cost) for m in want]
    # search_with_fn: the callback sees the pattern and the text as given
    keep = lambda p, t, strand: len(t) % 2 == 0  # noqa: E731
    got = ci.search_with_fn(pat, text, k, False, keep)
    same(got, oracle.search_modes("ascii", fold(pat), ft, k, end_filter=keep), "with_fn")
    # search_all_alignments against the helper on the folded inputs
    short = text[at - 200:at + 200]
    groups = ci.search_all_alignments(pat, short, k)
    assert aref.as_tuples(groups) == aref.search_all_alignments("ascii", fold(pat), fold(short), k) and groups
    # search_many / search_texts / search_patterns
    pats = [pat, swap_case(rng, text[300:340]), b"no such THING here"]
    texts = [text[i:i + 2100] for i in range(0, len(text), 2000)]

    def many(ps, ts, kk):
        return [(pi, ti) + key(m)[1:] for pi, p in enumerate(ps) for ti, t in enumerate(ts)
                for m in oracle.search("ascii", fold(p), fold(t), kk)]

    got = ci.search_many(pats, texts, 3)
    assert [(m.pattern_idx, m.text_idx) + key(m)[1:] for m in got] == many(pats, texts, 3) and got
    got = ci.search_texts(pat, texts, k)
    assert [(m.pattern_idx, m.text_idx) + key(m)[1:] for m in got] == many([pat], texts, k) and got
    same_len = [pat, swap_case(rng, text[900:924])]
    got = ci.search_patterns(same_len, dev, k)
    assert [(m.pattern_idx, m.text_idx) + key(m)[1:] for m in got] == many(same_len, [text], k) and got
    # min_costs / best_pattern / best_matches
    import numpy as np
    cost = ci.min_costs(pats, texts, 3)
    want_cost = np.full((len(pats), len(texts)), 255, dtype=np.uint8)
    for r in many(pats, texts, 3):
        want_cost[r[0], r[1]] = min(want_cost[r[0], r[1]], r[6])
    assert (cost == want_cost).all()
    bc, bp, _ = ci.best_pattern(pats, texts, 3)
    assert (bc == want_cost.min(axis=0)).all()
    assert all(bp[t] == int(np.argmin(want_cost[:, t])) for t in range(len(texts)) if bc[t] != 255)
    got = ci.best_matches(pats, texts, 3)
    want_best = bref.expected(lambda p, t: oracle.search("ascii", fold(p), fold(t), 3), pats, texts)
    assert [bref.got_record(m) for m in got] == want_best and got
    # search_shard, search_shard_begin / search_finish, merge
    n = len(text)
    halo = sassy.required_halo(len(pat), k)
    cut = 64 * 120
    r0 = ci.search_shard(pat, buf.ptr, 0, cut, 0, n, k)
    r1 = ci.search_shard(pat, buf.ptr + cut - halo, halo, n - cut, cut, n, k)
    same(sassy.merge_shards([r0, r1]).matches, want, "merge")
    t0 = ci.search_shard_begin(pat, buf.ptr, 0, n, 0, n, k)
    t1 = ci.search_shard_begin(pats[1], buf.ptr, 0, n, 0, n, k)
    same(ci.search_finish(t0).matches, want, "in flight 0")
    same(ci.search_finish(t1).matches, oracle.search("ascii", fold(pats[1]), ft, k), "in flight 1")
    # the drop-in search()
    L = sassy.lib()
    h = L.sassy_searcher(b"ASCII_CI", False, float("nan"))
    out = C.POINTER(sassy.CMatch)()
    cnt = L.search(h, pat, len(pat), text, len(text), k, C.byref(out))
    assert [(out[i].text_start, out[i].text_end, out[i].cost) for i in range(cnt)] == [(m.text_start, m.text_end, m.cost) for m in want]
    L.sassy_matches_free(out, cnt)
    L.sassy_searcher_free(h)
    # sassy_hip_format_tsv: the match region is the text as it stands
    m0, = ci.search(b"hello", b"they say HeLLo twice", 0)
    assert ci.format_tsv(m0, "p", "t", b"they say HeLLo twice") == "p\tt\t0\t+\t9\t14\tHeLLo\t5=\n"
    # the in-process multi-device searcher takes the name (one device: one shard)
    ms = sassy.MultiSearcher("ascii_ci", [0])
    ms.set_text(text, 64, 4)
    same(ms.search(pat, k).matches, want, "multi")
    buf.free()
