"""GPU: line resolution on the device (sassy_hip_line_spans, SASSY_HIP_LINE_SPANS) against tests/helpers/line_spans_ref.py,
and the agrep front end end to end."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import line_spans_ref as ref  # noqa: E402
from helpers import scan_levels as lv  # noqa: E402
from helpers.prose_text import fold, on_device, prose  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    assert sassy_amd.device_count() > 0, "no HIP device: the GPU tests must not silently skip"
    return sassy_amd


def want_spans(sassy, text, first, last):
    """The helper's spans as the structured array the library returns -- through numpy's newline positions, so that 10^5
    spans of a text of megabytes take no 10^5 passes over it (the definitions stay the helper's: a sample is compared
    with it one by one)."""
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10).astype(np.uint64)
    first, last = np.asarray(first, dtype=np.uint64), np.asarray(last, dtype=np.uint64)
    out = np.empty(len(first), dtype=sassy.line_span_dtype())
    ia, ib = np.searchsorted(nl, first, side="left"), np.searchsorted(nl, last, side="left")
    out["line_no"], out["last_line_no"] = ia + 1, ib + 1
    out["line_start"] = np.where(ia > 0, nl[np.maximum(ia, 1) - 1] + 1 if len(nl) else 0, 0)
    out["line_end"] = np.where(ib < len(nl), nl[np.minimum(ib, max(len(nl) - 1, 0))] if len(nl) else len(text), len(text))
    for i in list(range(min(len(first), 40))) + list(range(0, len(first), max(1, len(first) // 60))):
        assert tuple(int(x) for x in out[i]) == ref.line_span(text, int(first[i]), int(last[i])), i
    return out


def random_text(rng, n, density):
    """n bytes, each a newline with probability `density` (0: none, 1: all)."""
    a = np.frombuffer(rng.randbytes(n), dtype=np.uint8).copy() if n else np.zeros(0, dtype=np.uint8)
    a[a == 10] = 11
    if density >= 1:
        a[:] = 10
    elif density > 0:
        a[np.frombuffer(rng.randbytes(4 * n), dtype=np.uint32) < density * 2 ** 32] = 10
    return a.tobytes()


def random_spans(rng, n, count, tile):
    first = np.array([rng.randrange(n + 1) for _ in range(count)], dtype=np.uint64)
    width = np.array([rng.choice((0, 0, 1, 5, 80, 3 * tile, n)) for _ in range(count)], dtype=np.uint64)
    return first, np.minimum(first + width, n).astype(np.uint64)


def first_bad(got, want, first, last):
    """the first differing span: its index, its ends and the super-tiles (64 KiB) they lie in, what came and what was due"""
    i = int(np.flatnonzero(got != want)[0])
    return ("span", i, int(first[i]), int(last[i]), "super-tiles", int(first[i]) >> 16, int(last[i]) >> 16, "got", got[i], "want", want[i])


def check(sassy, s, text, first, last, dev=None):
    want = want_spans(sassy, text, first, last)
    got = s.line_spans(text, first, last)
    assert got.dtype == sassy.line_span_dtype()
    assert (got == want).all(), (np.flatnonzero(got != want)[:5], first_bad(got, want, first, last))
    if dev is not None:
        got = s.line_spans(dev, first, last)
        assert (got == want).all(), ("device text", np.flatnonzero(got != want)[:5], first_bad(got, want, first, last))


def test_random_texts_and_densities(sassy):
    rng = random.Random(4242)
    s = sassy.Searcher("ascii", rc=False)
    tile = sassy.line_tile()
    assert tile == 4096
    for n, density in ((0, 0), (1, 1), (1, 0), (63, 0.1), (tile - 1, 0.02), (tile, 0.02), (tile + 1, 0.5), (16 * tile, 0.0125),
                       (16 * tile + 5, 0), (70_001, 1), (300_000, 0.0125), (3_000_001, 0.0125), (2_500_000, 0), (1_000_000, 0.9)):
        text = random_text(rng, n, density)
        buf, dev = on_device(sassy, text) if n else (None, None)
        first, last = random_spans(rng, n, 200, tile)
        check(sassy, s, text, first, last, dev)
        if buf:
            buf.free()


def test_tile_borders_and_a_long_line(sassy):
    """Spans at the borders of the index's tiles (sassy_hip_line_tile) and super-tiles (16 tiles), newlines right at and
    next to them, and one line longer than 64 tiles with lines around it."""
    rng = random.Random(5)
    s = sassy.Searcher("ascii", rc=False)
    tile = sassy.line_tile()
    n = 40 * tile + 17
    a = np.full(n, ord("x"), dtype=np.uint8)
    borders = [t * tile for t in (1, 2, 3, 15, 16, 17, 31, 32, 33, 40)]
    for b in borders[::2]:
        a[b - 1] = 10
    for b in borders[1::2]:
        a[b] = 10
    a[5] = a[6] = 10
    text = a.tobytes()
    pos = sorted({min(max(b + d, 0), n) for b in borders + [0, n] for d in (-65, -64, -2, -1, 0, 1, 2, 63, 64, 65)})
    first = np.array([p for p in pos for _ in range(3)], dtype=np.uint64)
    last = np.minimum(first + np.array([0, 1, tile] * len(pos), dtype=np.uint64), n).astype(np.uint64)
    buf, dev = on_device(sassy, text)
    check(sassy, s, text, first, last, dev)
    buf.free()
    # one line of 70 tiles between short lines
    long_line = 70 * tile + 123
    text = b"first\nsecond\n" + b"y" * long_line + b"\nlast but one\nlast"
    n = len(text)
    inside = [13, 14, 13 + tile, 13 + 16 * tile - 1, 13 + 16 * tile, 13 + 33 * tile + 7, 13 + long_line - 1, 13 + long_line]
    first = np.array([0, 6, 12] + inside + [13 + long_line + 1, n - 4, n], dtype=np.uint64)
    check(sassy, s, text, first, first)
    got = s.line_spans(text, inside, inside)
    assert all(tuple(int(x) for x in g) == (3, 3, 13, 13 + long_line) for g in got)
    first, last = random_spans(rng, n, 300, tile)
    check(sassy, s, text, first, last)


def test_more_than_1024_super_tiles(sassy):
    """64 MiB + 4096 + 17 bytes (helpers/scan_levels.py: lines_big): n_super = 1025, so every thread of line_scan_kernel sums
    per = 2 super-tile counts (thread 512 one, the threads behind it none); the counts are very uneven -- 0, 65 536, about
    820 and 1150 -- so that a prefix shifted by one super-tile shows in every span behind it."""
    rng = random.Random(1025)
    s = sassy.Searcher("ascii", rc=False)
    text = lv.lines_big()
    n = len(text)
    n_super = -(-n // lv.SUPER)
    print(f"{n} bytes, n_super={n_super} per={-(-n_super // 1024)}")
    assert n_super == 1025
    first, last = lv.lines_spans()
    more_first, more_last = random_spans(rng, n, 300, sassy.line_tile())
    buf, dev = on_device(sassy, text)
    check(sassy, s, text, np.concatenate([first, more_first]), np.concatenate([last, more_last]), dev)
    buf.free()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 100_000])
def test_span_counts(sassy, count):
    rng = random.Random(count)
    s = sassy.Searcher("ascii", rc=False)
    text = random_text(rng, 1_500_000, 1 / 80)
    first = np.frombuffer(rng.randbytes(8 * count), dtype=np.uint64) % np.uint64(len(text) + 1)
    last = np.minimum(first + (np.frombuffer(rng.randbytes(8 * count), dtype=np.uint64) % np.uint64(200)), len(text)).astype(np.uint64)
    buf, dev = on_device(sassy, text)
    check(sassy, s, text, first, last, dev if count in (1, 100_000) else None)
    buf.free()


def test_argument_errors(sassy):
    s = sassy.Searcher("ascii", rc=False)
    assert len(s.line_spans(b"a\nb", [], [])) == 0      # n == 0
    assert len(s.line_spans(b"", [], [])) == 0
    assert [tuple(int(x) for x in r) for r in s.line_spans(b"", [0], [0])] == [(1, 1, 0, 0)]
    with pytest.raises(sassy.SassyHipError, match="libsassy_hip error -1"):
        s.line_spans(b"a\nb", [2], [1])
    with pytest.raises(sassy.SassyHipError, match="libsassy_hip error -1"):
        s.line_spans(b"a\nb", [0], [4])
    with pytest.raises(sassy.SassyHipError, match="libsassy_hip error -1"):
        s.line_spans(b"", [0], [1])


def test_search_with_line_spans(sassy):
    rng = random.Random(77)
    text = prose(rng, 200_000)
    at = 150_001
    cut = text[at:at + 18]
    assert sum(a != b for a, b in zip(cut, fold(cut))) > 4  # more capitals than the case-sensitive search has errors to spend
    buf, dev = on_device(sassy, text)
    for alphabet, k in (("ascii_ci", 2), ("ascii", 4)):
        s = sassy.Searcher(alphabet, rc=False)
        pat = fold(cut) if alphabet == "ascii_ci" else cut  # ascii: the text as it stands -- the folded cut is no match there
        for t in (text, dev):
            plain = s._search(pat, t, k, 0)
            r = s._search(pat, t, k, sassy.LINE_SPANS)
            assert r.matches == plain.matches and len(r) >= 1, alphabet
            first = r.array["text_start"]
            last = np.maximum(first, r.array["text_end"] - np.minimum(r.array["text_end"], 1))
            assert (r.line_spans == s.line_spans(t, first, last)).all()
            assert (r.line_spans == want_spans(sassy, text, first, last)).all()
            assert plain.line_spans is None
        ms, spans = s.search_lines(pat, text, k, all_minima=True)
        assert [(m.text_start, m.text_end, m.cost) for m in ms] == \
            [(m.text_start, m.text_end, m.cost) for m in oracle.search("ascii", fold(pat) if alphabet == "ascii_ci" else pat,
                                                                       fold(text) if alphabet == "ascii_ci" else text, k, all_minima=True)]
        assert [tuple(int(x) for x in sp) for sp in spans] == [ref.match_span(text, m.text_start, m.text_end) for m in ms]
    # a match across a newline
    s = sassy.Searcher("ascii_ci", rc=False)
    ms, spans = s.search_lines(b"two three", b"one two\nTHREE four\nfive", 1)
    assert [(m.text_start, m.text_end, m.cost) for m in ms] == [(4, 13, 1)]
    assert [tuple(int(x) for x in sp) for sp in spans] == [(1, 2, 0, 18)]
    # no match: an empty array, not None
    ms, spans = s.search_lines(b"absent", b"nothing\nhere", 0)
    assert ms == [] and spans is not None and len(spans) == 0
    # the flag belongs to sassy_hip_search alone
    L = sassy.lib()
    out = C.c_void_p()
    pp, pl = (C.c_char_p * 1)(pat), (C.c_size_t * 1)(len(pat))
    tp, tl = (C.c_void_p * 1)(buf.ptr), (C.c_size_t * 1)(len(text))
    assert L.sassy_hip_search_many(s._h, pp, pl, 1, tp, tl, 1, 1, sassy.LINE_SPANS | sassy.TEXT_ON_DEVICE, C.byref(out)) == -3
    d = sassy.Searcher("dna", rc=False)
    e = d.encode_patterns([b"ACGTACGT"])
    assert L.sassy_hip_search_encoded(d._h, e._h, buf.ptr, len(text), 1, sassy.LINE_SPANS | sassy.TEXT_ON_DEVICE, C.byref(out)) == -3
    buf.free()


def agrep_restated(name, text, pattern, k, ci, context):
    """The agrep output from the oracle's matches and the helper's spans, by lines split on the host."""
    ms = oracle.search("ascii", fold(pattern) if ci else pattern, fold(text) if ci else text, k)
    ms.sort(key=lambda m: (m.text_start, m.text_end))
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # a final newline opens no line
    out, shown = [], 0
    for i, m in enumerate(ms):
        l0, l1, a, b = ref.match_span(text, m.text_start, m.text_end)
        nxt = ref.match_span(text, ms[i + 1].text_start, ms[i + 1].text_end)[0] if i + 1 < len(ms) else None
        before = [x for x in range(max(1, l0 - context), l0) if x > shown]
        if context and shown and (before[0] if before else l0) > shown + 1:
            out.append("--\n")
        out += [f"{name}-{x}-{lines[x - 1].decode(errors='replace')}\n" for x in before]
        out.append(f"{name}:{l0}:{m.text_start - a + 1}:{m.cost}:{text[a:b].decode(errors='replace')}\n")
        shown = max(shown, l1)
        for x in range(l1 + 1, min(l1 + context, len(lines)) + 1):
            if nxt is not None and x >= nxt:
                break
            if x > shown:
                out.append(f"{name}-{x}-{lines[x - 1].decode(errors='replace')}\n")
                shown = x
    hist = [0] * (k + 1)
    for m in ms:
        hist[m.cost] += 1
    return "".join(out), hist


def run_cli(args, stdin=b""):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "sassy_amd", "agrep"] + args, input=stdin, cwd=ROOT, env=env, capture_output=True, timeout=300)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_agrep_end_to_end(sassy, tmp_path):
    from sassy_amd.cli import format_histogram
    rng = random.Random(11)
    text_a = prose(rng, 30_000).replace(b"\xe9", b"e")
    text_b = b"no newline at the end: Kernel timeout\n\nkernel TIMEOUT again\nKERNEL_TIMEOUT"
    a, b = tmp_path / "a.log", tmp_path / "b.log"
    a.write_bytes(text_a)
    b.write_bytes(text_b)
    pat = "lazy dog"
    for extra, ci, ctx in (([], False, 0), (["-i"], True, 0), (["-C", "1"], False, 1), (["-i", "-C", "2"], True, 2)):
        rc, out, err = run_cli(extra + [pat, "2", str(a)])
        want, hist = agrep_restated(str(a), text_a, pat.encode(), 2, ci, ctx)
        assert out == want and (rc == 0) == (sum(hist) > 0), (extra, rc, err[-300:])
        assert err.endswith(format_histogram(hist)), err[-300:]
        assert sum(hist) >= (3 if ci else 1), hist
    # two files, and stdin
    rc, out, err = run_cli(["-i", "-C", "1", "kernel timeout", "1", str(a), str(b)])
    wa, ha = agrep_restated(str(a), text_a, b"kernel timeout", 1, True, 1)
    wb, hb = agrep_restated(str(b), text_b, b"kernel timeout", 1, True, 1)
    assert rc == 0 and out == wa + wb and sum(hb) == 3
    assert err.endswith(format_histogram([x + y for x, y in zip(ha, hb)]))
    for args in (["kernel timeout", "0"], ["kernel timeout", "0", "-"]):
        rc, out, err = run_cli(args, stdin=text_b)
        assert rc == 1 and out == "" and err.endswith(format_histogram([0])), (rc, out, err)  # case-sensitive: nothing matches
    rc, out, err = run_cli(["-i", "kernel timeout", "0"], stdin=text_b)
    assert rc == 0 and out == agrep_restated("(stdin)", text_b, b"kernel timeout", 0, True, 0)[0]
    assert out == "(stdin):1:24:0:no newline at the end: Kernel timeout\n(stdin):3:1:0:kernel TIMEOUT again\n"
    rc, out, err = run_cli(["x", "0", str(tmp_path / "missing")])
    assert rc == 2 and out == ""
