"""GPU: every instantiation of the traceback (sassy_amd/csrc/trace_kernel.hip) with ascii, ascii_ci and class patterns, and
k >= 255 with every alphabet, against the oracle.

tests/helpers/trace_shapes.py names the kernel that runs for (m, k, options, reports, texts) and builds the inputs;
tests/test_trace_shapes_cpu.py ties both to the sources and checks every input's conditions with the oracle alone.  Here
the device's records must equal the oracle's field by field, cigar included: byte patterns on folded inputs, class patterns
whose sets are pairwise equal or disjoint on inputs mapped to representatives; class patterns of overlapping sets by the
report rule on the numpy last row and a replay of every record.  Options are per searcher (Searcher.set_option).

Not reachable through the public entry points, and so no case here: trace_kernel<uint16_t, true, -1> and
trace_wave_kernel<uint16_t, .> (64 slices of two-byte cells pass kTraceLdsLimit for every m >= 1, a band of 513 columns
is no wavefront's), and the thread kernel of many_patterns.hip for the ascii alphabets (the pattern-tiled and seeded paths
that end in it refuse ascii and ascii_ci: their lists of patterns run one ScanJob per pattern).  test_many_patterns reaches
that switch with dna and iupac and runs ascii_ci through search_many / search_patterns with the option on either side.

Wall time on the MI355X, one run of this file beside the traceback group of test_gpu_parity.py (pytest --durations=0; 49
tests in 9.9 s, the oracle's share included):
  test_window_boundary        0.53 / 0.50 s (dna, two routes), 0.28 s (classes), 0.24 s (ascii_ci)
  test_k255                   0.32 - 0.40 s (class patterns, two kinds), 0.12 - 0.15 s (dna, iupac), 0.08 s (ascii, ascii_ci)
  test_every_label            0.22 s (wave_k30, KT0 with the first searchers), 0.18 s (k = 31), 0.08 s and less elsewhere
  test_many_patterns          0.03 - 0.05 s;  test_several_texts: below 0.005 s
  for comparison, same run    test_dense_reports 0.84 s, test_traceback_variants 0.64 s (dna), 0.61 s (iupac)
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import classes_ref as cref  # noqa: E402
from helpers import trace_shapes as ts  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    assert sassy_amd.device_count() > 0, "no HIP device: the GPU tests must not silently skip"
    return sassy_amd


@pytest.fixture(scope="module")
def searchers(sassy):
    """One searcher per (alphabet, options): a fresh one only where an option differs."""
    made = {}

    def get(alphabet, options=None):
        k = (ts.SEARCHER[alphabet], tuple(sorted((options or {}).items())))
        if k not in made:
            s = sassy.Searcher(k[0], rc=False)
            for name, value in k[1]:
                s.set_option(name, value)
                assert s.get_option(name) == value
            made[k] = s
        return made[k]
    return get


def same(got, want, ctx):
    assert len(got) == len(want), (ctx, len(got), len(want), got[:3], want[:3])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (ctx, i, g, w)


def ends(ms):
    return [(m.text_end, m.cost) for m in ms]


def run(sassy, s, inp, text, all_minima=False, without_trace=False):
    if inp.kind == "bytes":
        assert not without_trace
        return s.search_all(inp.pattern, text, inp.k) if all_minima else s.search(inp.pattern, text, inp.k)
    return s.search_classes(ts.pattern_of(inp, sassy), text, inp.k, all_minima=all_minima, without_trace=without_trace)


def check(sassy, s, inp, text, all_minima, ctx):
    """One search against its reference; class patterns also without_trace beside it."""
    got = run(sassy, s, inp, text, all_minima)
    want = ts.expected(inp, text, all_minima)
    want_ends = ts.expected_ends(inp, text, all_minima) if want is None else [(w[1], w[4]) for w in want]
    if want is not None:
        same([ts.key(m) for m in got], want, ctx)
    else:
        same(ends(got), want_ends, ctx)
        sets = ts.effective_sets(inp)
        for m in got:
            cref.replay(sets, text, m)
    if inp.kind != "bytes":
        same(ends(run(sassy, s, inp, text, all_minima, without_trace=True)), want_ends, ctx + ("without trace",))
    return got


# ---------------------------------------------------------------- every label of the table
@pytest.mark.parametrize("case", ts.TABLE, ids=[c.name for c in ts.TABLE])
def test_every_label(sassy, searchers, case):
    for inp in ts.table_inputs(case):
        s = searchers(inp.alphabet, case.options)
        ctx = (case.name, case.want, inp.alphabet, inp.kind)
        got = check(sassy, s, inp, inp.text, False, ctx + ("search",))
        assert len(got) >= 4
        check(sassy, s, inp, inp.text[:inp.prefix], True, ctx + ("search_all",))


# ---------------------------------------------------------------- several texts: the rank kernels with report_text
@pytest.mark.parametrize("alphabet,case,want", ts.texts_cases(), ids=[f"{a}-{c.name}" for a, c, _ in ts.texts_cases()])
def test_several_texts(sassy, searchers, alphabet, case, want):
    s = searchers(alphabet, case.options)
    inp = ts.build(alphabet, case.m, case.k, seed=77)
    texts = ts.cut_texts(inp)
    got = s.search_texts(inp.pattern, texts, inp.k)
    same([(m.pattern_idx, m.text_idx) + ts.key(m) for m in got], ts.expected_texts(inp, texts), (alphabet, case.name, want))


# ---------------------------------------------------------------- many patterns: both sides of the thread-kernel switch
@pytest.mark.parametrize("alphabet", ["ascii_ci", "dna", "iupac"])
def test_many_patterns(sassy, alphabet):
    pats, texts, want = ts.many_case(alphabet)
    s = sassy.Searcher(ts.SEARCHER[alphabet], rc=False)
    if alphabet != "ascii_ci":
        s.set_option("many_tiled", 1)  # the one-pass paths, whose report list trace_reports (many_patterns.hip) traces
    assert len(want) >= ts.MANY_THREADS
    results = []
    for threads in (ts.MANY_THREADS, 0):  # the thread kernel from 64 reports on; never
        s.set_option("encoded_trace_threads", threads)
        got = [(m.pattern_idx, m.text_idx) + ts.key(m) for m in s.search_many(pats, texts, ts.MANY_K)]
        if alphabet != "ascii_ci":
            assert s.stats()["filtered"] in (5, 6), s.stats()["filtered"]  # the pattern-tiled scan or the seeded search
        same(got, want, (alphabet, "search_many", threads))
        one = [(m.pattern_idx, m.text_idx) + ts.key(m) for m in s.search_patterns(pats, texts[0], ts.MANY_K)]
        same(one, [w for w in want if w[1] == 0], (alphabet, "search_patterns", threads))
        results.append((got, one))
    assert results[0] == results[1]


# ---------------------------------------------------------------- the window boundary
@pytest.mark.parametrize("k", ts.BOUNDARY_KS)
@pytest.mark.parametrize("alphabet", ts.BOUNDARY_ALPHABETS)
def test_window_boundary(sassy, searchers, alphabet, k):
    """8191, 8192, 8193 and 8200 records: either side of the two kernels' count windows.  Before each, a search with more
    and different records on the same searcher: a row no kernel wrote would carry that search's content."""
    # the count the kernels' windows test is the device list's.  Under the fused bit-plane filter (dna at its default
    # route) that list holds copies the dedup removes later, so the streaming DP (prefilter = 0) is what makes the count
    # exact there; the default route runs beside it, records compared all the same
    routes = [({"prefilter": 0}, True), ({}, False)] if alphabet == "dna" else [({}, True)]
    for options, exact in routes:
        s = searchers(alphabet, options)
        for count in ts.BOUNDARY_COUNTS:
            before = ts.boundary_case(alphabet, k, count + 40, seed=1, m=ts.BOUNDARY_M - 1)
            assert len(run(sassy, s, before, before.text, True)) == count + 40
            inp = ts.boundary_case(alphabet, k, count)
            want = ts.boundary_expected(inp)
            assert len(want) == count
            got = run(sassy, s, inp, inp.text, True)
            st = s.stats()
            if exact:
                assert st["fused"] == 0 and st["candidates"] == count, st  # no copies: the list's count is the records'
            same([ts.key(m) for m in got], want, (alphabet, k, count, options, ts.label(inp.m, k, None, count)))


# ---------------------------------------------------------------- k >= 255: two-byte cells
@pytest.mark.parametrize("k", ts.K255)
@pytest.mark.parametrize("alphabet", sorted(ts.K255_M))
def test_k255(sassy, searchers, alphabet, k):
    """k = 254 still has one-byte cells (k + 1 = 255 is the largest value a cell holds), 255 and 256 two-byte cells; the
    expected records hold costs up to k -- at k = 256 one above 255, where a one-byte cell wraps."""
    s = searchers(alphabet)
    for kind in ts.KINDS[alphabet]:
        inp = ts.k255_case(alphabet, k, kind)
        got = check(sassy, s, inp, inp.text, False, (alphabet, kind, k, ts.K255_WANT[k]))
        assert max(m.cost for m in got) == k
