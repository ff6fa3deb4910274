"""GPU: character-class patterns (Searcher.search_classes / sassy_hip_search_classes).

Where a class pattern says the same as a byte pattern of an existing alphabet -- singleton sets (ascii), case twins
(ascii_ci), base sets over ACGT text (iupac), or sets that partition the bytes so that text and pattern can be mapped to
representatives -- the records must equal the oracle's field by field, cigar included: the DP, the report rule and the
traceback's tie-breaks see only the match relation.  General sets are checked against the numpy restatement
(helpers/classes_ref.py): the (text_end, cost) list of the report rule on its last row, and every record replayed."""
import io
import os
import random
import sys

import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import classes_ref as cref  # noqa: E402
from helpers import line_spans_ref as lref  # noqa: E402
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


def ends(ms):
    return [(m.text_end, m.cost) for m in ms]


def mutate(rng, s, edits, alphabet=b"abcXYZ_@[ \n\xe9"):
    s = bytearray(s)
    for _ in range(edits):
        t, p = rng.randrange(3), rng.randrange(len(s))
        if t == 0:
            s[p] = rng.choice(alphabet)
        elif t == 1:
            s.insert(p, rng.choice(alphabet))
        elif len(s) > 1:
            del s[p]
    return bytes(s)


def check_against_reference(s, sets, text, k, ctx=None, sets_seen=None):
    """search, search_all and without_trace of the class pattern `sets` against the numpy reference: the end positions
    and costs of the report rule, and every traced record replayed.  sets_seen: the sets the searcher really compares
    with (ascii_ci: closed under case).  Returns the matches of `search`."""
    import sassy_amd
    pat = sassy_amd.ClassPattern.from_sets(sets)
    eff = sets if sets_seen is None else sets_seen
    row = cref.last_row(eff, text)
    out = None
    for all_minima in (False, True):
        want = oracle.find_ends(row, k, all_minima)
        got = s.search_classes(pat, text, k, all_minima=all_minima)
        assert ends(got) == want, (ctx, all_minima, ends(got)[:5], want[:5], len(got), len(want))
        for m in got:
            cref.replay(eff, text, m)
        wt = s.search_classes(pat, text, k, all_minima=all_minima, without_trace=True)
        assert ends(wt) == want, (ctx, "without trace", all_minima)
        if not all_minima:
            out = got
    return out


# ------------------------------------------------------------------ 1. singletons = ascii
def test_singletons_equal_ascii(sassy):
    rng = random.Random(20261017)
    s = sassy.Searcher("ascii", rc=False)
    text = prose(rng, 24_000)
    buf, dev = on_device(sassy, text)
    total = costly = 0
    for m in (1, 2, 31, 32, 33, 63, 64, 65, 66, 129, 300):
        for k in sorted({0, 1, m // 6, m // 3}):
            while True:  # the prose has more than 64 distinct bytes, a class pattern at most 64 distinct sets
                at = rng.randrange(0, len(text) - m)
                pat = text[at:at + m]
                if k and m > 3:
                    pat = mutate(rng, pat, rng.randrange(1, k + 1))
                if len(set(pat)) <= 64:
                    break
            cp = sassy.ClassPattern.from_sets([[c] for c in pat])
            # texts of a size the oracle's naive DP takes quickly for long patterns
            lo = 0 if m <= 66 else max(0, at - 3000) // 16 * 16
            t = text if m <= 66 else text[lo:at + 3000]
            d = dev if m <= 66 else type(dev)(buf.ptr + lo, len(t))
            want = oracle.search("ascii", pat, t, k)
            same(s.search_classes(cp, t, k), want, ("search", m, k))
            same(s.search_classes(cp, d, k), want, ("search, device text", m, k))
            total += len(want)
            costly += sum(1 for x in want if x.cost > 0)
            ta = t[:6000]
            want_all = oracle.search("ascii", pat, ta, k, all_minima=True)
            same(s.search_classes(cp, ta, k, all_minima=True), want_all, ("all", m, k))
            same(s.search_classes(cp, type(dev)(buf.ptr + lo, len(ta)), k, all_minima=True), want_all, ("all, device text", m, k))
            assert ends(s.search_classes(cp, t, k, without_trace=True)) == ends(want), ("without trace", m, k)
            assert ends(s.search_classes(cp, d, k, without_trace=True)) == ends(want), ("without trace, device text", m, k)
    buf.free()
    assert total >= 15 and costly >= 3, (total, costly)


# ------------------------------------------------------------------ 2. case twins = ascii_ci
def swap_case(rng, s, p=0.5):
    return bytes((c ^ 0x20) if (chr(c).isascii() and chr(c).isalpha() and rng.random() < p) else c for c in s)


def test_case_twins_equal_ascii_ci(sassy):
    rng = random.Random(42)
    cs = sassy.Searcher("ascii", rc=False)
    ci = sassy.Searcher("ascii_ci", rc=False)
    text = prose(rng, 12_000)  # holds '_@[', newlines and bytes >= 0x80
    assert all(c in text for c in b"_@[\n\xe9\xff")
    ft = fold(text)
    n = 0
    for m, k in ((1, 0), (5, 1), (20, 3), (33, 2), (64, 6), (65, 0), (130, 12)):
        at = rng.randrange(0, len(text) - m)
        pat = swap_case(rng, text[at:at + m])
        if k:
            pat = mutate(rng, pat, rng.randrange(0, k + 1))
        twins = [[c, c ^ 0x20] if chr(c).isascii() and chr(c).isalpha() else [c] for c in pat]
        for all_minima in (False, True):
            t, f = (text, ft) if not all_minima else (text[:5000], ft[:5000])
            want = oracle.search("ascii", fold(pat), f, k, all_minima=all_minima)
            same(cs.search_classes(sassy.ClassPattern.from_sets(twins), t, k, all_minima=all_minima), want, ("twins", m, k, all_minima))
            same(ci.search_classes(sassy.ClassPattern.from_sets([[c] for c in pat]), t, k, all_minima=all_minima), want,
                 ("ascii_ci, singletons", m, k, all_minima))
            n += len(want) if not all_minima else 0
    assert n >= 7
    # only letters have a twin: '@' / '`', '[' / '{' and 0xC9 / 0xE9 differ in bit 5 alone
    for a, b in ((b"@", b"`"), (b"[", b"{"), (b"\xc9", b"\xe9")):
        assert ci.search_classes(sassy.ClassPattern.from_sets([a]), b"xx" + b + b"xx", 0) == []
        assert len(ci.search_classes(sassy.ClassPattern.from_sets([a]), b"xx" + a + b"xx", 0)) == 1
    assert len(ci.search_classes(b"[k-m]ernel", b"say KERNEL and Lernel", 0)) == 2


# ------------------------------------------------------------------ 3. base sets over ACGT = iupac
IUPAC_SETS = {"A": b"A", "C": b"C", "G": b"G", "T": b"T", "R": b"AG", "Y": b"CT", "S": b"CG", "W": b"AT", "K": b"GT",
              "M": b"AC", "B": b"CGT", "D": b"AGT", "H": b"ACT", "V": b"ACG", "N": b"ACGT"}


def test_base_sets_equal_iupac(sassy):
    rng = random.Random(3)
    s = sassy.Searcher("ascii", rc=False)
    text = bytearray(rng.choice(b"ACGT") for _ in range(20_000))
    pats = ["ACGTNNRYACGTBACGT", "".join(IUPAC_SETS), "GATTACANNNNNRYSWKMBDHVTTGACC" * 2, "NRYH"]
    for i, p in enumerate(pats):  # an instance of every pattern, some edited
        inst = bytes(rng.choice(IUPAC_SETS[c]) for c in p)
        at = 1000 + 4000 * i
        text[at:at + len(inst)] = inst
        inst2 = mutate(rng, inst, 2, b"ACGT")
        text[at + 2000:at + 2000 + len(inst2)] = inst2
    text = bytes(text)
    assert set(text) == set(b"ACGT")
    n = 0
    for p in pats:
        cp = sassy.ClassPattern.from_sets([IUPAC_SETS[c] for c in p])
        for k in (0, 2) if len(p) > 4 else (0,):
            want = oracle.search("iupac", p.encode(), text, k)
            assert want, (p, k)
            same(s.search_classes(cp, text, k), want, ("iupac", p, k))
            ta = text[:6000] if len(p) > 4 else text[:800]
            same(s.search_classes(cp, ta, k, all_minima=True), oracle.search("iupac", p.encode(), ta, k, all_minima=True), ("iupac all", p, k))
            n += len(want)
    assert n >= 8


# ------------------------------------------------------------------ 4. general sets
def mapped(text: bytes, groups):
    """Every byte of a group replaced by the group's first byte (groups: disjoint bytes objects)."""
    tab = bytearray(range(256))
    for g in groups:
        for c in g:
            tab[c] = g[0]
    return bytes(text).translate(bytes(tab))


def test_parsed_expressions(sassy):
    s = sassy.Searcher("ascii", rc=False)
    text = (b"The grey cat and the gray dog met a groy fox on 2026-10-17,\nnot on 2026/10/17 or 202X-10-17.\n"
            b"gr\ny is split; g.ay is dotted.\nab cd  ef\n") * 3
    # sets that are pairwise equal or disjoint: the oracle on mapped inputs gives the records
    want = oracle.search("ascii", b"gray", mapped(text, [b"ae"]), 1)
    got = s.search_classes(b"gr[ae]y", text, 1)
    same(got, want, "gr[ae]y")
    assert sum(1 for m in got if m.cost == 0) == 6 and any(m.cost == 1 for m in got)
    date = rb"\d\d\d\d-\d\d-\d\d"
    want = oracle.search("ascii", b"0000-00-00", mapped(text, [b"0123456789"]), 2)
    got = s.search_classes(date, text, 2)
    same(got, want, "date")
    assert sorted(m.cost for m in got)[:9] == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    same(s.search_classes(date, text, 2, all_minima=True), oracle.search("ascii", b"0000-00-00", mapped(text, [b"0123456789"]), 2, all_minima=True), "date all")
    # '.' is every byte but the newline; [^ ] every byte but the blank
    got = s.search_classes(b"gr.y", text, 0)
    assert [text[m.text_start:m.text_end] for m in got] == [b"grey", b"gray", b"groy"] * 3
    got = s.search_classes(b"g.ay", text, 0)
    assert [text[m.text_start:m.text_end] for m in got] == [b"gray", b"g.ay"] * 3
    for expr, k in ((b"[^ ][^ ][^ ][^ ][^ ][^ ][^ ]", 0), (b"[^ ][^ ] [^ ][^ ]  ", 1), (b"t.\n.o", 1), (rb"\w\w\W\s\S.", 2)):
        p = sassy.parse_classes(expr)
        check_against_reference(s, [p.members(j) for j in range(p.m)], text, k, expr)


def test_random_sets(sassy):
    rng = random.Random(77)
    s = sassy.Searcher("ascii", rc=False)
    ci = sassy.Searcher("ascii_ci", rc=False)
    seen_inv = 0
    for densities in ([1, 2, 3, 16, 64, 240, 254, 255], [128, 8, 100, 200]):  # (two patterns: each inside the cube cap)
        sets = [frozenset(rng.sample(range(256), d)) for d in densities]
        sets.insert(2, frozenset())            # a position nothing matches
        sets.insert(4, frozenset(range(256)))  # a position everything matches
        covers = [sassy.class_cover(x) for x in sets]
        seen_inv += sum(inv for _, inv in covers)
        assert sum(len(c) for c, _ in covers) <= sassy.CLASS_MAX_CUBES
        text = bytearray(rng.randrange(256) for _ in range(9000))
        for at in (0, 50, 1000, 4090, 9000 - len(sets)):  # instances (the empty set's position costs one edit)
            inst = bytes(rng.choice(sorted(x)) if x else 0x55 for x in sets)
            text[at:at + len(inst)] = inst
        text = bytes(text)
        for k in (1, 3):
            got = check_against_reference(s, sets, text, k, ("random", densities, k))
            assert len(got) >= 4
        # the same through an ascii_ci searcher: the sets it compares with are closed under case
        got = check_against_reference(ci, sets, text, 2, ("random, ascii_ci", densities), sets_seen=cref.close_case(sets))
        assert len(got) >= 4
    assert seen_inv >= 4  # slots stored as their complement


# ------------------------------------------------------------------ 5. slots and cubes
def test_slot_counts(sassy):
    rng = random.Random(5)
    s = sassy.Searcher("ascii", rc=False)
    alphabet = list(range(33, 127))
    for n in (1, 16, 17, 64):  # (17: more slots than the Ascii prefilters carry)
        letters = rng.sample(alphabet, n)
        pat = bytes(letters) if n > 1 else bytes(letters) * 9
        text = bytearray(rng.choice(alphabet) for _ in range(5000))
        text[700:700 + len(pat)] = pat
        text[3000:3000 + len(pat)] = pat
        if n > 1:
            text[3000 + len(pat) // 2] ^= 1
        text = bytes(text)
        k = 0 if n == 1 else 2
        cp = sassy.ClassPattern.from_sets([[c] for c in pat])
        want = oracle.search("ascii", pat, text, k)
        assert len(want) >= 2
        same(s.search_classes(cp, text, k), want, ("slots", n))
        # the same number of slots with sets of two and three bytes
        sets = [frozenset([c, c ^ 0x80, (c + 1) ^ 0x80]) for c in pat]
        check_against_reference(s, sets, text, k, ("slots, wider sets", n))
    with pytest.raises(sassy.SassyHipError, match="64 distinct sets"):
        s.search_classes(sassy.ClassPattern.from_sets([[c] for c in range(65)]), b"some text", 0)


def test_cube_cap(sassy):
    s = sassy.Searcher("ascii", rc=False)
    # bytes four apart are 64 runs of one: 64 cubes, and the complement's runs of three take two each
    quarter = [frozenset(range(t, 256, 4)) for t in range(4)]
    for q in quarter:
        cubes, inv = sassy.class_cover(q)
        assert len(cubes) == 64 and not inv
    assert 4 * 64 == sassy.CLASS_MAX_CUBES
    rng = random.Random(8)
    text = bytes(rng.randrange(256) for _ in range(4000))
    sets = quarter + quarter[::-1] + quarter  # twelve rows, four slots, 256 cubes
    got = check_against_reference(s, sets, text, 5, "at the cap")
    assert got
    with pytest.raises(sassy.SassyHipError, match="256 cubes"):
        s.search_classes(sassy.ClassPattern.from_sets(sets + [b"a"]), text, 5)


def test_what_is_refused(sassy):
    cp = sassy.parse_classes(b"gr[ae]y")
    text = b"a grey day, then rain. " * 40
    for alphabet in ("dna", "iupac"):
        with pytest.raises(sassy.SassyHipError, match="ascii"):
            sassy.Searcher(alphabet, rc=False).search_classes(cp, text, 0)
    with pytest.raises(sassy.SassyHipError, match="reverse complement"):
        sassy.Searcher("ascii", rc=True).search_classes(cp, text, 0)
    with pytest.raises(sassy.SassyHipError):
        sassy.Searcher("iupac", rc=False, alpha=0.5).search_classes(cp, text, 0)
    s = sassy.Searcher("ascii", rc=False)
    with pytest.raises(sassy.SassyHipError, match="empty"):
        s.search_classes(sassy.ClassPattern(b""), text, 0)
    with pytest.raises(sassy.SassyHipError):  # line spans need traced matches, as for search
        s.search_classes(cp, text, 0, without_trace=True, lines=True)
    # the calls that take byte patterns only say so
    buf, dev = on_device(sassy, text)
    calls = [
        lambda: s.search(cp, text, 0), lambda: s.search_all(cp, text, 0), lambda: s.search_lines(cp, text, 0),
        lambda: s.search_all_alignments(cp, text, 0), lambda: s.search_with_fn(cp, text, 0, False, lambda *a: True),
        lambda: s.search_many([cp], [text], 0), lambda: s.min_costs([cp], [text], 0), lambda: s.best_pattern([cp], [text], 0),
        lambda: s.best_matches([cp], [text], 0), lambda: s.encode_patterns([cp]), lambda: s.search_patterns([cp], text, 0),
        lambda: s.search_texts(cp, [text], 0), lambda: s.search_shard(cp, buf.ptr, 0, len(text), 0, len(text), 0),
        lambda: s.search_shard_begin(cp, buf.ptr, 0, len(text), 0, len(text), 0),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(sassy.SassyHipError, match="byte patterns only"):
            call()
    ms = sassy.MultiSearcher("ascii", [0])
    ms.set_text(text, 16, 1)
    with pytest.raises(sassy.SassyHipError, match="byte patterns only"):
        ms.search(cp, 0)
    buf.free()
    assert [m.cigar for m in s.search_classes(cp, text, 0)] == ["4="] * 40  # and the searcher still works


# ------------------------------------------------------------------ 6. geometry
@pytest.fixture(scope="module")
def long_pattern():
    """300 rows (ten 32-row words): digit and letter ranges, twins, a complement, '.'-like rows."""
    rng = random.Random(300)
    kinds = [frozenset(b"0123456789"), frozenset(range(97, 123)), frozenset(b"aeiouAEIOU"), frozenset(range(256)) - {10},
             frozenset(range(256)) - frozenset(b" \n"), frozenset(b"xX"), frozenset(b"_"), frozenset(b"kK")]
    sets = [rng.choice(kinds) for _ in range(300)]

    def instance(edits=0):
        inst = bytes(rng.choice(sorted(x - {10, 32})) for x in sets)
        return mutate(rng, inst, edits, b"q7_ ")
    return sets, instance


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 300_011])
def test_geometry(sassy, long_pattern, n):
    sets, instance = long_pattern
    rng = random.Random(n)
    s = sassy.Searcher("ascii", rc=False)
    text = bytearray(prose(rng, n))
    plants = []
    if n >= 4095:
        # at offset 0, across 64-byte block boundaries, and at the very end; in the long text also around the chunk seams
        plants = [(0, 0), (1000, 7), (64 * 40 - 150, 12), (n - 300, 0)]
        if n > 100_000:
            plants += [(at, e) for at, e in ((64 * 777 - 17, 3), (150_000, 25), (222_222, 0), (n - 700, 30))]
    for at, e in plants:
        inst = instance(e)
        inst = inst[:n - at]
        text[at:at + len(inst)] = inst
    text = bytes(text)[:n]
    pat = sassy.ClassPattern.from_sets(sets)
    row = cref.last_row(sets, text)
    buf, dev = on_device(sassy, text)
    s.text_unchanged(True)
    for k in (0, 30):
        want = oracle.find_ends(row, k)
        got = s.search_classes(pat, text, k)
        assert ends(got) == want, (n, k, ends(got)[:4], want[:4])
        for m in got:
            cref.replay(sets, text, m)
        # the same device text again and again (SASSY_HIP_TEXT_UNCHANGED)
        same(s.search_classes(pat, dev, k), got, ("device", n, k))
        assert ends(s.search_classes(pat, dev, k, without_trace=True)) == want
        want_all = oracle.find_ends(row, k, True)
        assert ends(s.search_classes(pat, dev, k, all_minima=True, without_trace=True)) == want_all, (n, k, "all")
        if n >= 4095:
            assert len(want) >= (2 if k == 0 else len(plants) - 1), (n, k, want)
    buf.free()


# ------------------------------------------------------------------ 7. lines and the agrep front end
def test_lines(sassy):
    rng = random.Random(12)
    s = sassy.Searcher("ascii", rc=False)
    text = prose(rng, 30_000) + b"\nrelease 2026-10-17 and 2026-1O-18\n\nlast 1999-12-31"
    for expr, k in ((rb"\d\d\d\d-\d\d-\d\d", 1), (b"[Kk]ernel.[a-z][a-z]", 1), (b"dog\n[A-Z]", 0)):
        ms, spans = s.search_classes(expr, text, k, lines=True)
        assert ms and len(spans) == len(ms)
        assert [tuple(int(x) for x in sp) for sp in spans] == [lref.match_span(text, m.text_start, m.text_end) for m in ms], expr
        same(ms, s.search_classes(expr, text, k), expr)
    ms, spans = s.search_classes(b"[xyz]bsent", b"nothing\nhere", 0, lines=True)
    assert ms == [] and spans is not None and len(spans) == 0


def run_agrep(argv, stdin=b""):
    from sassy_amd.cli import agrep_parser, run_agrep as run
    out, err = io.StringIO(), io.StringIO()
    rc = run(agrep_parser().parse_args(argv), stdin=io.BytesIO(stdin), out=out, err=err)
    return rc, out.getvalue(), err.getvalue()


def reference_spans(text, ms):
    return [dict(zip(("line_no", "last_line_no", "line_start", "line_end"), lref.match_span(text, m.text_start, m.text_end))) for m in ms]


def test_agrep_classes(sassy, tmp_path):
    from sassy_amd.cli import format_agrep, format_histogram
    rng = random.Random(13)
    text = (prose(rng, 6000).replace(b"\xe9", b"e") + b"\nbuilt 2026-10-17, shipped 2026-1x-19\nGREY skies\ngray seas, groy?\n" +
            prose(rng, 3000).replace(b"\xe9", b"e") + b"\nno newline at the end: grEy")
    path = tmp_path / "notes.txt"
    path.write_bytes(text)
    digits = [b"0123456789"]
    for argv, pat, groups, ci, k, ctx in (
            (["-E", r"\d\d\d\d-\d\d-\d\d", "1"], b"0000-00-00", digits, False, 1, 0),
            (["--classes", "-C", "1", r"\d\d\d\d-\d\d-\d\d", "1"], b"0000-00-00", digits, False, 1, 1),
            (["-E", "gr[ae]y", "0"], b"gray", [b"ae"], False, 0, 0),
            (["-E", "-i", "gr[ae]y s", "1"], b"gray s", [b"ae"], True, 1, 0),
            (["-i", "-E", "-C", "2", "GR[AE]Y", "0"], b"gray", [b"ae"], True, 0, 2)):
        rc, out, err = run_agrep(argv + [str(path)])
        t = mapped(fold(text) if ci else text, groups)
        want = oracle.search("ascii", pat, t, k)
        assert want, argv
        assert out == format_agrep(str(path), text, want, reference_spans(text, want), ctx), (argv, err[-300:])
        hist = [sum(1 for m in want if m.cost == c) for c in range(k + 1)]
        assert rc == 0 and err.endswith(format_histogram(hist)), (argv, err[-300:])
    # -i matches across case, the plain search does not
    assert "GREY skies" in run_agrep(["-E", "-i", "gr[ae]y", "0", str(path)])[1]
    assert "GREY skies" not in run_agrep(["-E", "gr[ae]y", "0", str(path)])[1]
    rc, out, err = run_agrep(["-E", "gr[ae]y", "0"], stdin=b"a GRAY day\n")
    assert rc == 1 and out == ""
    rc, out, err = run_agrep(["-E", "gr[ae", "0", str(path)])
    assert rc == 2 and "unterminated" in err
    # without -E the brackets are bytes of the pattern
    rc, out, err = run_agrep(["gr[ae]y", "0"], stdin=b"grey gr[ae]y\n")
    assert rc == 0 and out == "(stdin):1:6:0:grey gr[ae]y\n"
