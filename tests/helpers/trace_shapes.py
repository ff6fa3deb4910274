"""The traceback's kernel family restated in plain Python, the table of shapes that reaches every member of it, and the
inputs the tests of those shapes share.  No device.

Part 1 restates what the host decides (sassy_amd/csrc/host_internal.h::trace_shape, scan_route.h / scan_driver.hip,
trace_kernel.hip::launch_trace, many_patterns.hip::trace_reports): from (m, k), the searcher's options, the number of
reports and of texts to a label naming the instantiation that traces them.  tests/test_trace_shapes_cpu.py reads the
constants out of the sources and compares.

Part 2 is the case table: per label the smallest (m, k) the rule allows above a floor that is written down (m_floor).

Part 3 builds the inputs: mixed-case prose with plants of 0 .. k edits (substitutions, insertions and deletions), one
instance cut by the text's start and one by its end, for byte patterns, class patterns whose sets partition the bytes, and
class patterns of overlapping sets -- with the expectation of each from the oracle."""
import os
import random
import sys
from collections import namedtuple
from types import SimpleNamespace

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classes_ref as cref  # noqa: E402
from prose_text import fold, prose  # noqa: E402

# ---------------------------------------------------------------- 1. the rule
TRACE_WAVE_MAX = 8192          # ScanJob::kTraceWaveMax
TRACE_LDS_LIMIT = 128 * 1024   # kTraceLdsLimit
TRACE_WAVE_DUMMY = 128         # kTraceWaveDummy
WAVE_LDS = 160 * 1024          # a workgroup's LDS: four wave slices and their patterns must fit
KT_CASES = (0, 1, 2, 3, 4, 5, 6)  # launch_trace: the k with a register-band instantiation
ONE_BYTE_CELLS_MAX = 255       # cells are one byte while k + 1 <= 255
ENCODED_TRACE_THREADS = 65536  # many_patterns.hip: the thread kernel from this many reports on (option -1)
DEFAULTS = {"trace_wave": 1, "self_rank": 1, "encoded_trace_threads": -1}


def trace_shape(m, k):
    s = SimpleNamespace()
    s.cell = 1 if k + 1 <= ONE_BYTE_CELLS_MAX else 2
    s.band = ((m + 1) * (2 * k + 3) * s.cell + 3) // 4 * 4
    s.win = (m + k + 15 + 15) // 16 * 16
    s.ops = (m + k + 1 + 3) // 4 * 4
    s.str = (2 * (m + k + 1) + 2 + 15) // 16 * 16
    s.raw = s.band + s.win + s.ops + s.str
    s.pat_bytes = (m + 15) // 16 * 16
    s.wave_stride = (s.raw + TRACE_WAVE_DUMMY + 15) // 16 * 16
    s.thread_stride = s.raw + (4 if (s.raw // 4) % 2 == 0 else 0)
    s.wave_fits = 2 * k + 3 <= 64 and 4 * s.pat_bytes + 4 * s.wave_stride <= WAVE_LDS
    s.thread_in_lds = 64 * s.thread_stride + s.pat_bytes <= TRACE_LDS_LIMIT
    return s


def thread_label(m, k, overhang=False):
    ts = trace_shape(m, k)
    cell = "u8" if ts.cell == 1 else "u16"
    where = "lds" if ts.thread_in_lds else "global"
    if ts.cell == 1 and ts.thread_in_lds and not overhang and k in KT_CASES:
        return f"thread<u8,lds,KT={k}>"
    return f"thread<{cell},{where}>"


def label(m, k, options=None, n_reports=1, n_texts=1, many=False, overhang=False):
    """The instantiation that traces `n_reports` reports of a pattern of m rows at k.  many: the report list of many
    patterns (many_patterns.hip); else one ScanJob (scan_driver.hip), n_texts > 1: a multi-text buffer."""
    opt = dict(DEFAULTS)
    opt.update(options or {})
    ts = trace_shape(m, k)
    cell = "u8" if ts.cell == 1 else "u16"
    if many:
        assert 2 * k + 3 <= 64  # (the callers made sure)
        tt = opt["encoded_trace_threads"]
        start = tt if tt > 0 else ENCODED_TRACE_THREADS
        if tt != 0 and k <= 6 and not overhang and n_reports >= start and ts.thread_in_lds:
            return thread_label(m, k)
        return f"wave<{cell}>"
    use_wave = opt["trace_wave"] != 0 and ts.wave_fits
    use_thread = not use_wave or (k <= 6 and not overhang)
    self_rank = opt["self_rank"] != 0 and use_wave and n_texts == 1
    # the count windows: the wave kernel takes 0 < count <= kTraceWaveMax when the thread kernel is armed too (or when it
    # ranks its reports itself: beyond, the device sort runs first), the thread kernel kTraceWaveMax < count
    if use_wave and (not use_thread or n_reports <= TRACE_WAVE_MAX):
        ranked = "+self_rank" if self_rank and n_reports <= TRACE_WAVE_MAX else "+rank"
        return f"wave<{cell}>{ranked}"
    return thread_label(m, k, overhang)


# ---------------------------------------------------------------- 2. the case table
Case = namedtuple("Case", "name want m k options")


def m_floor(k):
    """A pattern shorter than about 2k matches unrelated prose within k nearly everywhere: nothing to tell apart."""
    return 2 * k + 8


def smallest_m(want, k, options=None, lo=None, hi=4096):
    for m in range(m_floor(k) if lo is None else lo, hi):
        if label(m, k, options) == want:
            return m
    raise AssertionError(f"no m gives {want} at k = {k}")


def largest_m(want, k, options=None, hi=4096):
    for m in range(hi, 0, -1):
        if label(m, k, options) == want:
            return m
    raise AssertionError(f"no m gives {want} at k = {k}")


NO_WAVE = {"trace_wave": 0}


def case_table():
    t = [Case(f"KT{k}", f"thread<u8,lds,KT={k}>", smallest_m(f"thread<u8,lds,KT={k}>", k, NO_WAVE), k, NO_WAVE) for k in KT_CASES]
    t.append(Case("lds_k7", "thread<u8,lds>", smallest_m("thread<u8,lds>", 7, NO_WAVE), 7, NO_WAVE))
    # k = 31 at default options: the band is 65 columns, no wave; 64 slices fit LDS only below the floor (k >= m there:
    # every window is a match) -- the largest m the rule allows says the most
    t.append(Case("lds_k31", "thread<u8,lds>", largest_m("thread<u8,lds>", 31), 31, {}))
    t.append(Case("global_k3", "thread<u8,global>", smallest_m("thread<u8,global>", 3, NO_WAVE), 3, NO_WAVE))
    t.append(Case("global_k31", "thread<u8,global>", smallest_m("thread<u8,global>", 31), 31, {}))
    for k in (7, 30):
        for sr in (1, 0):
            want = "wave<u8>+self_rank" if sr else "wave<u8>+rank"
            t.append(Case(f"wave_k{k}_sr{sr}", want, smallest_m(want, k, {"self_rank": sr}), k, {"self_rank": sr}))
    return t


TABLE = case_table()

# two-byte cells: m per alphabet, long enough that unrelated text does not lie within k = 256.  Decided with the oracle:
# the smallest multiple of 100 from 600 on at which the last row over 3000 bytes of unplanted background stays at or above
# K255_CLEAR = 1.25 * 256 (tests/test_trace_shapes_cpu.py checks both sides); random Dna needs the longest pattern
K255 = (254, 255, 256)
K255_WANT = {254: "thread<u8,global>", 255: "thread<u16,global>", 256: "thread<u16,global>"}
K255_CLEAR = 320
K255_M = {"ascii": 600, "ascii_ci": 600, "classes": 700, "classes_ci": 700, "dna": 700, "iupac": 700}

ALPHABETS = ("ascii", "ascii_ci", "classes", "classes_ci")
SEARCHER = {"ascii": "ascii", "ascii_ci": "ascii_ci", "classes": "ascii", "classes_ci": "ascii_ci", "dna": "dna", "iupac": "iupac"}

# ---------------------------------------------------------------- 3. inputs
# the bytes that differ from another byte of the text in bit 5 alone and are no letters: a fold applied to them, or to one
# side only, changes a cigar
SPECIALS = b"_@[\xc9"
TWINS = {0x5F: 0x7F, 0x40: 0x60, 0x5B: 0x7B, 0xC9: 0xE9}
# class patterns, sets that are pairwise equal or disjoint (also once closed under case): the oracle on mapped inputs
GROUPS = [b"abcdefghijklm", b"nopqrstuvwxyz", b"0123456789", b" \n"]
LOWER, UPPER = frozenset(range(97, 123)), frozenset(range(65, 91))
LOOSE = [frozenset(b"aeiouAEIOU"), LOWER, LOWER | UPPER, frozenset(b"0123456789_@["), frozenset(range(256)) - {10},
         frozenset(range(256)) - frozenset(b" \n"), frozenset(b" \n")]


def is_letter(c):
    return 65 <= c <= 90 or 97 <= c <= 122


def swap_case(rng, s, p=0.5):
    return bytes((c ^ 0x20) if (is_letter(c) and rng.random() < p) else c for c in s)


def mapped(text, groups=GROUPS):
    tab = bytearray(range(256))
    for g in groups:
        for c in g:
            tab[c] = g[0]
    return bytes(text).translate(bytes(tab))


def background(alphabet, rng, n):
    if alphabet in ("dna", "iupac"):
        return bytes(rng.choice(b"ACGT") for _ in range(n))
    return prose(rng, n)


def base_pattern(alphabet, rng, m):
    """The byte string every instance is made from."""
    if alphabet in ("dna", "iupac"):
        p = bytearray(rng.choice(b"ACGT") for _ in range(m))
        if alphabet == "iupac" and m >= 20:
            p[3], p[m // 2], p[m - 2] = ord("N"), ord("R"), ord("y")
        return bytes(p)
    p = bytearray(prose(rng, m + 40)[20:20 + m])
    if m >= 8:
        for i, c in enumerate(SPECIALS):
            p[(i + 1) * m // 5] = c
    return bytes(p)


def edited(alphabet, rng, inst, edits, kinds=(0, 1, 2)):
    """`edits` edits at positions spread over the instance, right to left: substitution, insertion, deletion in turn
    (kinds = (0,): substitutions only).  A substitution of a SPECIALS byte takes its bit-5 twin; any other a byte no
    pattern row of a byte pattern matches."""
    s = bytearray(inst)
    if edits <= 0 or len(s) < 3:
        return bytes(s)
    edits = min(edits, len(s) - 2)
    at = sorted(rng.sample(range(1, len(s) - 1), edits), reverse=True)
    dna = alphabet in ("dna", "iupac")
    for q, p in enumerate(at):
        kind = kinds[q % len(kinds)]
        if kind == 0:
            if dna:
                s[p] = rng.choice([c for c in b"ACGT" if c != s[p]])
            else:
                s[p] = TWINS.get(s[p], 0x23)
        elif kind == 1:
            s.insert(p, rng.choice(b"ACGT") if dna else 0x23)
        else:
            del s[p]
    return bytes(s)


def edited_specials_first(alphabet, rng, inst, edits, kinds=(0, 1, 2)):
    """As edited(); the first substitutions land on the SPECIALS bytes, so that their twins are in the text."""
    s = bytearray(inst)
    if alphabet in ("dna", "iupac") or edits <= 0:
        return edited(alphabet, rng, inst, edits, kinds)
    hit = [i for i, c in enumerate(s) if c in TWINS][:max(1, edits // 3)]
    for i in hit:
        s[i] = TWINS[s[i]]
    return edited(alphabet, rng, bytes(s), edits - len(hit), kinds)


Inputs = namedtuple("Inputs", "alphabet kind m k pattern sets text prefix plants")


def class_sets(alphabet, kind, base, rng):
    """Sets of a class pattern of which `base` is an instance.  partition: the GROUPS and singletons (under an ascii_ci
    searcher of the folded byte: its closure under case keeps them pairwise equal or disjoint); general: overlapping."""
    ci = alphabet == "classes_ci"
    sets = []
    for c in base:
        if kind == "partition":
            c = fold(bytes([c]))[0] if ci else c
            g = [x for x in GROUPS if c in x]
            sets.append(frozenset(g[0]) if g else frozenset([c]))
        else:
            r = rng.random()
            if is_letter(c):
                own = [s for s in LOOSE[:3] if c in s]
                sets.append(frozenset([c, c ^ 0x20]) if r < 0.6 else rng.choice(own) if r < 0.85 else LOOSE[5])
            else:
                own = [s for s in LOOSE[3:] if c in s]
                sets.append(frozenset([c]) if r < 0.5 else rng.choice(own))
    return sets


def vary(alphabet, rng, inst):
    """Another text the pattern matches at cost 0: case swapped (ascii_ci searchers), members of a partition's group
    exchanged (class patterns)."""
    s = bytes(inst)
    if alphabet in ("classes", "classes_ci"):
        s = bytes(rng.choice(g[0]) if (g := [x for x in GROUPS if c in x]) and rng.random() < 0.4 else c for c in s)
    if alphabet in ("ascii_ci", "classes_ci"):
        s = swap_case(rng, s)
    if alphabet in ("dna", "iupac"):
        s = bytes(c if c in b"ACGT" else {78: 65, 82: 65, 89: 67}[c] for c in s.upper())  # N, R -> A; Y -> C
    return s


def exact_instance(probe, rng, inst, cost):
    """`inst` with substitutions, one position after the other, until the pattern's best cost over it alone is `cost`
    (a substitution adds at most one; neighbouring edits and loose sets make some add nothing)."""
    s = bytearray(inst)
    free = list(range(1, len(s) - 1))
    rng.shuffle(free)
    dna = probe.alphabet in ("dna", "iupac")

    def put(p):
        s[p] = rng.choice([c for c in b"ACGT" if c != s[p]]) if dna else TWINS.get(s[p], 0x23)
    have = 0
    while free and have < cost:  # (as many more as are missing: never beyond `cost`)
        for _ in range(min(cost - have, len(free))):
            put(free.pop())
        have = int(last_row(probe, bytes(s)).min())
    return bytes(s)


def build(alphabet, m, k, seed, kind="bytes", levels=None, gap=None, last_exact=False):
    """Text = head (an instance cut by the text's start) | plants at `levels` edits | tail (cut by the text's end), prose
    (random bases) between; `prefix`: the length that holds the head and the first three plants, for search_all."""
    rng = random.Random(seed)
    base = base_pattern(alphabet, rng, m)
    sets = class_sets(alphabet, kind, base, rng) if kind != "bytes" else None
    if kind == "partition":  # (vary() exchanges members of a group; a general set's instance stays the base)
        def inst(e, kinds=(0, 1, 2)):
            return edited_specials_first(alphabet, rng, vary(alphabet, rng, base), e, kinds)
    elif kind == "general":
        def inst(e, kinds=(0, 1, 2)):
            return edited(alphabet, rng, swap_case(rng, base) if alphabet == "classes_ci" else base, e, kinds)
    else:
        def inst(e, kinds=(0, 1, 2)):
            return edited_specials_first(alphabet, rng, vary(alphabet, rng, base), e, kinds)
    if levels is None:
        levels = [0, min(k, 1), k // 2, k, max(k - 1, 0), min(k, 3), 0]
    gap = gap if gap is not None else m + k + 40
    cut0, cut1 = min(k, 2), min(k, 1)
    out = bytearray(inst(1 if k >= 3 else 0)[cut0:])
    plants = [(0, -1, len(out))]
    prefix = 0
    for i, e in enumerate(levels):
        out += background(alphabet, rng, gap + 17 * i)
        at = len(out)
        if last_exact and i == len(levels) - 1:
            probe = Inputs(alphabet, kind, m, k, base if kind == "bytes" else None, sets, b"", 0, [])
            out += exact_instance(probe, rng, inst(0), e)
        else:
            out += inst(e)
        plants.append((at, e, len(out)))
        if i == 2:
            prefix = len(out) + 10
    out += background(alphabet, rng, gap)
    at = len(out)
    tail = inst(1 if k >= 3 else 0)
    out += tail[:len(tail) - cut1]
    plants.append((at, -2, len(out)))
    pattern = base if kind == "bytes" else None
    return Inputs(alphabet, kind, m, k, pattern, sets, bytes(out), prefix or len(out), plants)


def key(r):
    return (r.text_start, r.text_end, r.pattern_start, r.pattern_end, r.cost, r.strand, r.cigar)


def expected(inp, text, all_minima=False):
    """The records the oracle gives (byte patterns, partitions): a list of key() tuples; None for general sets."""
    ci = SEARCHER[inp.alphabet] == "ascii_ci"
    f = fold if ci else bytes
    if inp.kind == "bytes":
        profile = inp.alphabet if inp.alphabet in ("dna", "iupac") else "ascii"
        return [key(r) for r in oracle.search(profile, f(inp.pattern), f(text), inp.k, all_minima=all_minima)]
    if inp.kind == "partition":
        rep = bytes(min(s) if len(s) > 1 else next(iter(s)) for s in inp.sets)
        return [key(r) for r in oracle.search("ascii", mapped(rep), mapped(f(text)), inp.k, all_minima=all_minima)]
    return None


def effective_sets(inp):
    return cref.close_case(inp.sets) if SEARCHER[inp.alphabet] == "ascii_ci" else inp.sets


def expected_ends(inp, text, all_minima=False):
    """(text_end, cost) of every record: from expected() or, general sets, the report rule on the numpy last row."""
    want = expected(inp, text, all_minima)
    if want is not None:
        return [(w[1], w[4]) for w in want]
    return oracle.find_ends(cref.last_row(effective_sets(inp), text), inp.k, all_minima)


def conditions(inp, ends, n):
    """What a case's expected records must hold (ends: (text_end, cost)): at least four, a cost 0 and (k > 0) a cost above
    it, one whose window is clipped by the text's start (text_end - (m + k) <= 0) and one that ends with the text."""
    assert len(ends) >= 4, (inp.alphabet, inp.kind, inp.m, inp.k, len(ends))
    assert any(c == 0 for _, c in ends), (inp.alphabet, inp.kind, inp.m, inp.k, "no cost 0")
    assert inp.k == 0 or any(c > 0 for _, c in ends), (inp.alphabet, inp.kind, inp.m, inp.k, "no cost > 0")
    assert any(e <= inp.m + inp.k for e, _ in ends), (inp.alphabet, inp.kind, inp.m, inp.k, "none clipped by the start")
    assert any(e == n for e, _ in ends), (inp.alphabet, inp.kind, inp.m, inp.k, "none at the end")


def cigar_ops(keys):
    return set(ch for w in keys for ch in w[6] if not ch.isdigit())


def pattern_of(inp, sassy=None):
    """What the search call takes: the bytes, or a ClassPattern of the sets."""
    return inp.pattern if inp.kind == "bytes" else sassy.ClassPattern.from_sets(inp.sets)


KINDS = {"ascii": ("bytes",), "ascii_ci": ("bytes",), "classes": ("partition", "general"), "classes_ci": ("partition", "general"),
         "dna": ("bytes",), "iupac": ("bytes",)}


def table_inputs(case):
    """Every (alphabet, kind) of the four text alphabets for one case of the table."""
    return [build(a, case.m, case.k, seed=1000 * case.k + case.m + 7 * i, kind=kind)
            for i, a in enumerate(ALPHABETS) for kind in KINDS[a]]


# ---------------------------------------------------------------- several texts
def cut_texts(inp):
    """The planted text cut into three texts of unequal length: in front of the last byte of the second plant and behind
    the first two of the last, unedited one (k permitting), so that windows clip at inner text borders: plants = (start,
    edits, end), the head first."""
    a = inp.plants[2][2] - min(inp.k, 1)
    b = inp.plants[7][0] + min(inp.k, 2)
    assert inp.plants[7][1] == 0
    return [inp.text[:a], inp.text[a:b], inp.text[b:]]


def expected_texts(inp, texts):
    return [(0, ti) + w for ti, t in enumerate(texts) for w in expected(inp, t)]


# ---------------------------------------------------------------- the window boundary
BOUNDARY_COUNTS = (8191, 8192, 8193, 8200)
BOUNDARY_KS = (3, 8)
BOUNDARY_ALPHABETS = ("dna", "ascii_ci", "classes")
BOUNDARY_M = 24


def boundary_case(alphabet, k, count, seed=0, m=BOUNDARY_M):
    """A pattern of one letter (in both cases; a class pattern of the two-byte set {a, b}) and a run of it: search_all
    reports every end position from m - k on, n - (m - k) + 1 records.  The length comes from the count."""
    rng = random.Random(seed + 31 * k + count)
    n = count + (m - k) - 1
    if alphabet == "dna":
        pat, sets, text = b"A" * m, None, bytes(rng.choice(b"Aa") for _ in range(n))
    elif alphabet == "ascii_ci":
        pat, sets, text = bytes(rng.choice(b"qQ") for _ in range(m)), None, bytes(rng.choice(b"qQ") for _ in range(n))
    else:
        pat, sets, text = None, [frozenset(b"ab")] * m, bytes(rng.choice(b"ab") for _ in range(n))
    kind = "bytes" if sets is None else "partition"
    return Inputs(alphabet, kind, m, k, pat, sets, text, n, [])


GROUPS_BOUNDARY = [b"ab"]


def boundary_expected(inp):
    if inp.kind == "bytes":
        return expected(inp, inp.text, True)
    return [key(r) for r in oracle.search("ascii", b"a" * inp.m, mapped(inp.text, GROUPS_BOUNDARY), inp.k, all_minima=True)]


# ---------------------------------------------------------------- k >= 255
def k255_case(alphabet, k, kind=None):
    """Plants at 0, about k / 2 and k edits of all kinds, and one whose cost is exactly k (exact_instance)."""
    m = K255_M[alphabet]
    kind = kind or KINDS[alphabet][0]
    return build(alphabet, m, k, seed=k * 7 + len(alphabet), kind=kind, levels=[0, k // 2, k, k - 1, k], gap=m // 2 + 60, last_exact=True)


def k255_background(alphabet, kind=None, seed=5):
    """Unplanted text and a pattern of the case's length: the oracle must find nothing within k = 256."""
    rng = random.Random(seed + 1)
    inp = build(alphabet, K255_M[alphabet], 256, seed=seed, kind=kind or KINDS[alphabet][0], levels=[], gap=10)
    return inp._replace(text=background(alphabet, rng, 3000))


def last_row(inp, text):
    """The last DP row of a case's pattern over `text`, by the reference of its kind."""
    f = fold if SEARCHER[inp.alphabet] == "ascii_ci" else bytes
    if inp.kind == "general":
        return cref.last_row(effective_sets(inp), text)
    if inp.kind == "partition":
        return oracle.last_row("ascii", mapped(bytes(min(s) for s in inp.sets)), mapped(f(text)))
    return oracle.last_row(inp.alphabet if inp.alphabet in ("dna", "iupac") else "ascii", f(inp.pattern), f(text))


# ---------------------------------------------------------------- the groups of cases, as both test files walk them
def by_name(name):
    return next(c for c in TABLE if c.name == name)


def texts_cases():
    """(alphabet, case, options, label with three texts): a KT shape and a wave shape; a multi-text buffer never ranks
    itself, so the wave shape runs behind the rank kernels with report_text."""
    out = []
    for a in ("ascii", "ascii_ci"):
        for name in ("KT3", "wave_k7_sr1"):
            c = by_name(name)
            out.append((a, c, label(c.m, c.k, c.options, n_texts=3)))
    return out


MANY_M, MANY_K, MANY_THREADS = 32, 3, 64


def many_case(alphabet, n=8):
    """n patterns of one length, each planted in a text of its own: (patterns, texts, expected (pattern_idx, text_idx) +
    key() in pattern-major order)."""
    inps = [build(alphabet, MANY_M, MANY_K, seed=400 + 13 * i) for i in range(n)]
    pats, texts = [x.pattern for x in inps], [x.text for x in inps]
    want = []
    for pi, x in enumerate(inps):
        for ti, t in enumerate(texts):
            want += [(pi, ti) + w for w in expected(x, t)]
    return pats, texts, want
