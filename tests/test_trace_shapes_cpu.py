"""No GPU: tests/helpers/trace_shapes.py against the sources it restates, its case table against its own rule, and the
inputs of tests/test_gpu_trace_shapes.py against the conditions they are built for -- by the oracle alone, before any
device sees them.  Whoever retunes kTraceWaveMax, kTraceLdsLimit or the list of register-band kernels gets a failing test
here, not a GPU test that silently traces through another kernel."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import trace_shapes as ts  # noqa: E402

CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, pattern):
    found = re.findall(pattern, text)
    assert len(found) >= 1 and len(set(found)) == 1, (pattern, found)
    return found[0]


def constants(host=None, common=None, trace=None):
    host, common, trace = host or source("host_internal.h"), common or source("common.h"), trace or source("trace_kernel.hip")
    a, b = constant(common, r"kTraceLdsLimit = (\d+) \* (\d+);")
    cases = re.findall(r"case (\d+): launch_one<uint8_t, true, (\d+)>", trace)
    assert cases and all(x == y for x, y in cases)
    return {"wave_max": int(constant(host, r"kTraceWaveMax = (\d+);")), "lds_limit": int(a) * int(b),
            "wave_dummy": int(constant(common, r"kTraceWaveDummy = (\d+);")), "kt": tuple(int(x) for x, _ in cases),
            "one_byte_max": int(constant(host, r"cell = \(k \+ 1 <= (\d+)\) \? 1 : 2;"))}


def test_the_restatement_uses_the_sources_constants():
    c = constants()
    assert c == {"wave_max": ts.TRACE_WAVE_MAX, "lds_limit": ts.TRACE_LDS_LIMIT, "wave_dummy": ts.TRACE_WAVE_DUMMY,
                 "kt": ts.KT_CASES, "one_byte_max": ts.ONE_BYTE_CELLS_MAX}
    trace, host, driver, route, many, switches = (source(n) for n in ("trace_kernel.hip", "host_internal.h", "scan_driver.hip",
                                                                     "scan_route.h", "many_patterns.hip", "switches.h"))
    # the cell rule, at the host and at both dispatches of launch_trace
    assert "if (P.k + 1 <= %d) {" % ts.ONE_BYTE_CELLS_MAX in trace and "if (P.k + 1 > %d) {" % ts.ONE_BYTE_CELLS_MAX in trace
    # trace_shape, line by line
    for line in ("s.band = ((uint64_t)(m + 1) * (2ull * k + 3) * cell + 3) / 4 * 4;",
                 "s.win = ((uint64_t)m + k + 15 + 15) / 16 * 16;",
                 "s.ops = ((uint64_t)m + k + 1 + 3) / 4 * 4;",
                 "s.str = (2ull * (m + k + 1) + 2 + 15) / 16 * 16;",
                 "s.raw = s.band + s.win + s.ops + s.str;",
                 "s.pat_bytes = ((uint64_t)m + 15) / 16 * 16;",
                 "s.wave_stride = (s.raw + kTraceWaveDummy + 15) / 16 * 16;",
                 "s.thread_stride = s.raw + ((s.raw / 4) % 2 == 0 ? 4 : 0);",
                 "s.wave_fits = 2ull * k + 3 <= 64 && 4 * s.pat_bytes + 4 * s.wave_stride <= 160 * 1024;",
                 "const uint64_t wg_bytes = 64 * s.thread_stride + s.pat_bytes;",
                 "s.thread_in_lds = wg_bytes <= kTraceLdsLimit;"):
        assert line in host, line
    assert ts.WAVE_LDS == 160 * 1024
    # launch_trace decides "in LDS" from the same sum
    assert "const size_t lds = (size_t)64 * P.scratch_stride + ((P.m + 15) / 16) * 16;" in trace
    assert "const bool in_lds = lds <= kTraceLdsLimit;" in trace
    # the selection rule
    assert "const bool use_wave = in.do_trace && sw.trace_wave != 0 && in.wave_fits;" in route
    assert "use_thread = !use_wave || (k <= 6 && !overhang);" in driver
    assert "self_rank = env_selfrank != 0 && do_trace && use_wave && texts.n == 0;" in driver
    assert "T.count_min = use_wave ? kTraceWaveMax : 0;" in driver
    assert "Tw.count_max = use_thread ? kTraceWaveMax : 0xFFFFFFFFu;" in driver
    assert "if (self_rank) Tw.count_max = kTraceWaveMax;" in driver
    assert "counts[0] > kTraceWaveMax && (use_thread || self_rank)" in driver
    assert "const uint32_t from = env_tt > 0 ? (uint32_t)env_tt : %du;" % ts.ENCODED_TRACE_THREADS in many
    assert "if (!env_off && k <= 6 && !T.use_alpha && n_rep >= from && ts.thread_in_lds) {" in many
    assert max(ts.KT_CASES) == 6
    for name, value in ts.DEFAULTS.items():
        assert re.search(r"X\(%s, %d," % (name, value), switches), name


def test_a_shape_matches_the_struct_by_hand():
    """m = 20, k = 3 worked by hand from host_internal.h"""
    s = ts.trace_shape(20, 3)
    assert (s.cell, s.band, s.win, s.ops, s.str) == (1, 192, 48, 24, 64)  # 21 * 9 = 189 -> 192; 53 -> 48; 24; 50 -> 64
    assert s.raw == 328 and s.thread_stride == 332 and s.wave_stride == 464 and s.pat_bytes == 32  # 82 words: even -> + 4
    assert s.wave_fits and s.thread_in_lds
    s = ts.trace_shape(1, 255)
    assert s.cell == 2 and s.band == 2 * 513 * 2 and not s.wave_fits and not s.thread_in_lds


def test_every_case_carries_its_label():
    names = [c.name for c in ts.TABLE]
    assert len(set(names)) == len(names)
    for c in ts.TABLE:
        assert ts.label(c.m, c.k, c.options) == c.want, c
    want = {f"thread<u8,lds,KT={k}>" for k in range(7)} | {"thread<u8,lds>", "thread<u8,global>", "wave<u8>+self_rank", "wave<u8>+rank"}
    assert {c.want for c in ts.TABLE} == want
    by = {c.name: c for c in ts.TABLE}
    # the smallest m above the floor; the global shapes are the first m at which 64 slices pass the limit
    for c in ts.TABLE:
        if c.name == "lds_k31":
            assert ts.label(c.m + 1, c.k, c.options) == "thread<u8,global>" and c.m < c.k
        elif c.name.startswith("global"):
            below = ts.label(c.m - 1, c.k, c.options)
            assert c.m == ts.m_floor(c.k) or (c.m > ts.m_floor(c.k) and below == f"thread<u8,lds,KT={c.k}>"), c
        else:
            assert c.m == ts.m_floor(c.k)
    assert by["global_k3"].k <= 6 and by["global_k31"].k >= 31 and by["lds_k7"].k == 7 and by["lds_k31"].options == {}
    assert all(c.options == {"trace_wave": 0} for c in ts.TABLE if c.name.startswith("KT") or c.name in ("lds_k7", "global_k3"))
    # the same shapes at default options run the wave kernel: the option is what reaches the thread kernels
    assert all(ts.label(c.m, c.k).startswith("wave<u8>") for c in ts.TABLE if c.options == {"trace_wave": 0})
    # two-byte cells
    for a, m in ts.K255_M.items():
        assert [ts.label(m, k) for k in ts.K255] == [ts.K255_WANT[k] for k in ts.K255], a
    assert [ts.trace_shape(700, k).cell for k in ts.K255] == [1, 2, 2]


def test_the_two_byte_kernel_in_lds_cannot_be_reached():
    """64 slices of two-byte cells pass kTraceLdsLimit for every m >= 1: trace_kernel<uint16_t, true, -1> and both
    trace_wave_kernel<uint16_t, .> (a band of 513 columns is no wavefront's) are no case of the table."""
    for k in (255, 256, 1000):
        assert not ts.trace_shape(1, k).thread_in_lds and not ts.trace_shape(1, k).wave_fits
        assert ts.label(1, k) == "thread<u16,global>"


def test_a_retuned_constant_moves_a_case(monkeypatch):
    for name, value in (("TRACE_LDS_LIMIT", 64 * 1024), ("TRACE_LDS_LIMIT", 256 * 1024), ("KT_CASES", (0, 1, 2, 3)),
                        ("ONE_BYTE_CELLS_MAX", 256)):
        with monkeypatch.context() as mp:
            mp.setattr(ts, name, value)
            moved = [c.name for c in ts.TABLE if ts.label(c.m, c.k, c.options) != c.want]
            moved += [k for k in ts.K255 if ts.label(700, k) != ts.K255_WANT[k]]
            assert moved, (name, value)
    # and read out of a retuned source the constants no longer equal the helper's
    retuned = source("host_internal.h").replace("kTraceWaveMax = 8192;", "kTraceWaveMax = 4096;")
    assert constants(host=retuned)["wave_max"] != ts.TRACE_WAVE_MAX


def test_the_count_windows():
    m, k = ts.BOUNDARY_M, ts.BOUNDARY_KS
    assert 0 <= k[0] <= 6 and 7 <= k[1] <= 30
    W = ts.TRACE_WAVE_MAX
    assert [ts.label(m, k[0], None, n) for n in ts.BOUNDARY_COUNTS] == ["wave<u8>+self_rank"] * 2 + [f"thread<u8,lds,KT={k[0]}>"] * 2
    assert [ts.label(m, k[1], None, n) for n in ts.BOUNDARY_COUNTS] == ["wave<u8>+self_rank"] * 2 + ["wave<u8>+rank"] * 2
    assert ts.BOUNDARY_COUNTS[:3] == (W - 1, W, W + 1)
    # several texts never rank themselves; many patterns switch by the option
    assert ts.label(22, 7, None, 10, n_texts=3) == "wave<u8>+rank"
    assert [x[2] for x in ts.texts_cases()] == ["thread<u8,lds,KT=3>", "wave<u8>+rank"] * 2
    M, K, T = ts.MANY_M, ts.MANY_K, ts.MANY_THREADS
    assert ts.label(M, K, {"encoded_trace_threads": T}, T, many=True) == f"thread<u8,lds,KT={K}>"
    assert ts.label(M, K, {"encoded_trace_threads": T}, T - 1, many=True) == "wave<u8>"
    assert ts.label(M, K, {"encoded_trace_threads": 0}, 10 ** 6, many=True) == "wave<u8>"
    assert ts.label(M, K, None, 65535, many=True) == "wave<u8>" and ts.label(M, K, None, 65536, many=True) == f"thread<u8,lds,KT={K}>"


# ---------------------------------------------------------------- the inputs, by the oracle alone
@pytest.mark.parametrize("case", ts.TABLE, ids=[c.name for c in ts.TABLE])
def test_table_inputs_meet_their_conditions(case):
    for inp in ts.table_inputs(case):
        assert len(inp.text) <= 4000 and inp.prefix < len(inp.text)
        ends = ts.expected_ends(inp, inp.text)
        ts.conditions(inp, ends, len(inp.text))
        assert len(ts.expected_ends(inp, inp.text[:inp.prefix], True)) >= 4
        if inp.sets:
            assert len(set(inp.sets)) <= 64  # a class pattern's distinct sets
        if inp.kind != "general":
            assert [(w[1], w[4]) for w in ts.expected(inp, inp.text)] == ends
        if SPECIAL_ALPHABET(inp):
            assert all(c in inp.pattern for c in ts.SPECIALS)
            assert any(t in inp.text for t in ts.TWINS.values()) or case.k == 0


def SPECIAL_ALPHABET(inp):
    return inp.alphabet == "ascii_ci" and inp.kind == "bytes"


def test_groups_hold_every_cigar_operation_and_swapped_case():
    ops = set()
    for case in ts.TABLE:
        for inp in ts.table_inputs(case):
            want = ts.expected(inp, inp.text)
            if want is not None:
                ops |= ts.cigar_ops(want)
            if inp.alphabet in ("ascii_ci", "classes_ci") and inp.kind == "bytes":
                # the plants differ from the pattern in case: the case-sensitive oracle finds fewer
                exact = ts.expected(inp._replace(alphabet="ascii"), inp.text)
                assert len(exact) < len(want) or sum(w[4] for w in exact) > sum(w[4] for w in want), case.name
    assert ops == set("=XID")
    ops = set()
    for a, c, _ in ts.texts_cases():
        inp = ts.build(a, c.m, c.k, seed=77)
        texts = ts.cut_texts(inp)
        want = ts.expected_texts(inp, texts)
        assert len({len(t) for t in texts}) == 3 and all(any(w[1] == ti for w in want) for ti in range(3))
        # windows clip at inner text borders: a record ends with a text that is not the last, one starts within m + k of a later text's start
        assert any(w[1] < 2 and w[3] == len(texts[w[1]]) for w in want) and any(w[1] > 0 and w[3] <= c.m + c.k for w in want), (a, c.name)
        assert any(w[6] == 0 for w in want) and any(w[6] > 0 for w in want)
        ops |= ts.cigar_ops([w[2:] for w in want])
    assert ops == set("=XID")
    for a in ("ascii_ci", "dna", "iupac"):
        pats, texts, want = ts.many_case(a)
        assert len({len(p) for p in pats}) == 1 and len(want) >= ts.MANY_THREADS and len(texts) >= 2
        assert ts.cigar_ops([w[2:] for w in want]) == set("=XID")
        assert all(any(w[0] == pi for w in want) for pi in range(len(pats)))


@pytest.mark.parametrize("alphabet", ts.BOUNDARY_ALPHABETS)
def test_boundary_counts_are_exact(alphabet):
    for k in ts.BOUNDARY_KS:
        for count in ts.BOUNDARY_COUNTS:
            inp = ts.boundary_case(alphabet, k, count)
            want = ts.boundary_expected(inp)
            assert len(want) == count and len(inp.text) <= 8300, (alphabet, k, count, len(want))
            assert want[-1][1] == len(inp.text) and want[0][1] == inp.m - k
            before = ts.boundary_case(alphabet, k, count + 40, seed=1, m=inp.m - 1)
            stale = ts.boundary_expected(before)
            assert len(stale) == count + 40 and all(a[:2] != b[:2] or a[6] != b[6] for a, b in zip(stale, want))
    if alphabet == "classes":
        assert all(len(s) == 2 for s in inp.sets)


@pytest.mark.parametrize("alphabet", sorted(ts.K255_M))
def test_k255_inputs(alphabet):
    m = ts.K255_M[alphabet]
    for kind in ts.KINDS[alphabet]:
        # unrelated text does not lie within k, and one step shorter it comes closer than the margin (or m is the floor)
        bg = ts.k255_background(alphabet, kind)
        assert int(ts.last_row(bg, bg.text).min()) >= ts.K255_CLEAR, (alphabet, kind)
    if m > 600:
        saved = ts.K255_M[alphabet]
        try:
            ts.K255_M[alphabet] = m - 100
            assert min(int(ts.last_row(bg, bg.text).min()) for bg in (ts.k255_background(alphabet, kind) for kind in ts.KINDS[alphabet])) < ts.K255_CLEAR
        finally:
            ts.K255_M[alphabet] = saved
    assert 600 <= m <= 1200
    costs = []
    for kind in ts.KINDS[alphabet]:
        for k in ts.K255:
            inp = ts.k255_case(alphabet, k, kind)
            assert len(inp.text) <= 8000
            ends = ts.expected_ends(inp, inp.text)
            ts.conditions(inp, ends, len(inp.text))
            assert any(c == k for _, c in ends) and any(k // 3 < c < 2 * k // 3 for _, c in ends), (alphabet, kind, k)
            if k == 256:
                assert any(c > 255 for _, c in ends)
            costs += [c for _, c in ends]
            if kind != "general":
                assert ts.cigar_ops(ts.expected(inp, inp.text)) == set("=XID")
    assert any(c < 255 for c in costs) and any(c == 255 for c in costs) and any(c > 255 for c in costs)
