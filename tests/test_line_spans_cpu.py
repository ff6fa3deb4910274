"""CPU-only: the line-span ABI's host side (symbols, struct layout, argument checks that need no device), the reference
helper the GPU tests compare against, and the agrep front end's pure host logic (arguments, block formatting)."""
import ctypes as C
import io
import os
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import line_spans_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def sassy():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


def test_symbols_and_layout(sassy):
    from test_cabi_symbols import declared_symbols
    L = sassy.lib()
    decl = declared_symbols()
    new = {"sassy_hip_line_spans", "sassy_hip_result_line_spans", "sassy_hip_line_tile", "sassy_hip_line_span_times"}
    assert new <= decl and new <= set(sassy.EXPORTED_SYMBOLS)
    for name in decl:
        assert hasattr(L, name), name
    assert set(sassy.EXPORTED_SYMBOLS) >= decl
    assert C.sizeof(sassy.LineSpan) == 32
    assert sassy.line_span_dtype().itemsize == 32
    assert sassy.line_span_dtype().names == ("line_no", "last_line_no", "line_start", "line_end")
    assert [getattr(sassy.LineSpan, f).offset for f, _ in sassy.LineSpan._fields_] == [0, 8, 16, 24]
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    assert "#define SASSY_HIP_LINE_SPANS 16u" in hdr and sassy.LINE_SPANS == 16
    assert f"#define SASSY_HIP_LINE_TILE {sassy.line_tile()}u" in hdr


def test_argument_checks_need_no_device(sassy):
    s = sassy.Searcher("ascii", rc=False)
    # n == 0 succeeds without a launch (and so without a device)
    assert len(s.line_spans(b"a\nb", [], [])) == 0
    with pytest.raises(sassy.SassyHipError, match="first <= last <= text_len"):
        s.line_spans(b"a\nb", [2], [1])
    with pytest.raises(sassy.SassyHipError, match="first <= last <= text_len"):
        s.line_spans(b"a\nb", [0, 1], [1, 4])
    # the flag is sassy_hip_search's alone: refused before any device work
    L = sassy.lib()
    out = C.c_void_p()
    pp, pl = (C.c_char_p * 1)(b"ab"), (C.c_size_t * 1)(2)
    tp, tl = (C.c_void_p * 1)(C.cast(C.c_char_p(b"xxabxx"), C.c_void_p).value), (C.c_size_t * 1)(6)
    assert L.sassy_hip_search_many(s._h, pp, pl, 1, tp, tl, 1, 0, sassy.LINE_SPANS, C.byref(out)) == -3
    assert b"sassy_hip_search only" in L.sassy_hip_last_error()
    assert L.sassy_hip_search_all_alignments(s._h, b"ab", 2, tp[0], 6, 0, sassy.LINE_SPANS, C.byref(out)) == -3
    assert L.sassy_hip_search_shard(s._h, b"ab", 2, 64, 0, 6, 0, 6, 0, sassy.LINE_SPANS, C.byref(out)) == -3
    d = sassy.Searcher("dna", rc=False)
    e = d.encode_patterns([b"ACGT"])
    assert L.sassy_hip_search_encoded(d._h, e._h, tp[0], 6, 0, sassy.LINE_SPANS, C.byref(out)) == -3
    assert L.sassy_hip_search(s._h, b"ab", 2, tp[0], 6, 0, sassy.LINE_SPANS | sassy.WITHOUT_TRACE, C.byref(out)) == -3


def test_reference_helper_on_hand_written_cases():
    # an empty text: one empty line
    assert ref.line_span(b"", 0, 0) == (1, 1, 0, 0)
    # no newline at all
    t = b"hello world"
    assert ref.line_span(t, 0, 0) == (1, 1, 0, 11)
    assert ref.line_span(t, 3, 7) == (1, 1, 0, 11)
    assert ref.line_span(t, 11, 11) == (1, 1, 0, 11)  # the empty span at n
    # a newline at 0 and at n - 1
    t = b"\nab\n"
    assert ref.line_span(t, 0, 0) == (1, 1, 0, 0)     # the newline itself belongs to the line it ends
    assert ref.line_span(t, 1, 2) == (2, 2, 1, 3)
    assert ref.line_span(t, 3, 3) == (2, 2, 1, 3)
    assert ref.line_span(t, 4, 4) == (3, 3, 4, 4)     # behind the final newline: an empty third line
    # consecutive newlines
    t = b"a\n\n\nb"
    assert ref.line_span(t, 1, 1) == (1, 1, 0, 1)
    assert ref.line_span(t, 2, 2) == (2, 2, 2, 2)
    assert ref.line_span(t, 3, 3) == (3, 3, 3, 3)
    assert ref.line_span(t, 4, 4) == (4, 4, 4, 5)
    # a span that crosses lines
    t = b"one\ntwo\nthree"
    assert ref.line_span(t, 2, 5) == (1, 2, 0, 7)
    assert ref.line_span(t, 0, 12) == (1, 3, 0, 13)
    assert ref.line_span(t, 3, 4) == (1, 2, 0, 7)
    # matches: [start, end) -> [start, max(start, end - 1)]
    assert ref.match_span(t, 4, 7) == (2, 2, 4, 7)
    assert ref.match_span(t, 4, 8) == (2, 2, 4, 7)    # the match ends with the newline: still line 2
    assert ref.match_span(t, 4, 9) == (2, 3, 4, 13)
    assert ref.match_span(t, 13, 13) == (3, 3, 8, 13)  # an empty match at n
    assert ref.line_spans(t, [0, 4], [0, 4]) == [(1, 1, 0, 3), (2, 2, 4, 7)]


def _m(start, end, cost=0):
    return SimpleNamespace(text_start=start, text_end=end, cost=cost)


def _spans(sassy, text, matches):
    import numpy as np
    return np.array([ref.match_span(text, m.text_start, m.text_end) for m in matches], dtype=sassy.line_span_dtype())


def test_agrep_arguments():
    sys.path.insert(0, ROOT)
    from sassy_amd.cli import agrep_parser
    a = agrep_parser().parse_args(["-i", "-C", "2", "needle", "1", "a.txt", "b.txt"])
    assert (a.ignore_case, a.context, a.pattern, a.k, a.paths) == (True, 2, "needle", 1, ["a.txt", "b.txt"])
    a = agrep_parser().parse_args(["needle", "0"])
    assert (a.ignore_case, a.context, a.paths) == (False, 0, [])
    with pytest.raises(SystemExit):
        agrep_parser().parse_args(["needle"])
    with pytest.raises(SystemExit):
        agrep_parser().parse_args(["needle", "x"])


def test_agrep_blocks(sassy):
    from sassy_amd.cli import format_agrep, format_histogram
    text = b"alpha\nbeta\ngamma\ndelta\nepsilon\nzeta\neta\ntheta\n"
    #        0      6     11     17     23       31    36   40
    ms = [_m(25, 28, 1), _m(7, 9, 0)]  # unsorted on purpose: "sil" in epsilon, "et" in beta
    sp = _spans(sassy, text, ms)
    assert format_agrep("f", text, ms, sp) == "f:2:2:0:beta\nf:5:3:1:epsilon\n"
    # -C 1: context rows; the two blocks touch (lines 3 and 4), so no separator stands between them, as in grep
    assert format_agrep("f", text, ms, sp, 1) == ("f-1-alpha\nf:2:2:0:beta\nf-3-gamma\n"
                                                 "f-4-delta\nf:5:3:1:epsilon\nf-6-zeta\n")
    # ... and one between blocks that do not touch
    far = [_m(7, 9, 0), _m(40, 45, 0)]
    assert format_agrep("f", text, far, _spans(sassy, text, far), 1) == ("f-1-alpha\nf:2:2:0:beta\nf-3-gamma\n--\n"
                                                                        "f-7-eta\nf:8:1:0:theta\n")
    # -C 2: the contexts meet (lines 3, 4 once each), no separator
    assert format_agrep("f", text, ms, sp, 2) == ("f-1-alpha\nf:2:2:0:beta\nf-3-gamma\nf-4-delta\n"
                                                 "f:5:3:1:epsilon\nf-6-zeta\nf-7-eta\n")
    # overlapping contexts of neighbours and two matches in one line: every match has its row, a line is context once,
    # and never behind its own match row
    ms = [_m(7, 9), _m(12, 14), _m(14, 16)]  # beta; "am" and "ma" in gamma
    sp = _spans(sassy, text, ms)
    assert format_agrep("f", text, ms, sp, 1) == ("f-1-alpha\nf:2:2:0:beta\nf:3:2:0:gamma\nf:3:4:0:gamma\nf-4-delta\n")
    # a match across a newline shows both lines; the context goes around them
    ms = [_m(9, 13, 2)]  # "a\nga"
    sp = _spans(sassy, text, ms)
    assert tuple(sp[0]) == (2, 3, 6, 16)
    assert format_agrep("f", text, ms, sp, 1) == "f-1-alpha\nf:2:4:2:beta\ngamma\nf-4-delta\n"
    # the edges of the text: no line in front of the first, none behind the final newline; bytes that are no UTF-8
    text2 = b"caf\xe9\nlast"
    ms = [_m(0, 3), _m(5, 9)]
    sp = _spans(sassy, text2, ms)
    assert format_agrep("p", text2, ms, sp, 3) == "p:1:1:0:caf\ufffd\np:2:1:0:last\n"
    ms = [_m(40, 45)]
    sp = _spans(sassy, text, ms)
    assert format_agrep("f", text, ms, sp, 1) == "f-7-eta\nf:8:1:0:theta\n"
    assert format_agrep("f", text, [], _spans(sassy, text, []), 2) == ""
    assert format_histogram([3, 0, 12]) == "\nStatistics: total 15\ndist:  0  1  2 \ncnt:   3  0 12 \n"


def test_agrep_reports_errors_with_status_2(sassy, tmp_path):
    from sassy_amd.cli import agrep_parser, run_agrep
    out, err = io.StringIO(), io.StringIO()
    args = agrep_parser().parse_args(["needle", "1", str(tmp_path / "missing.txt")])
    assert run_agrep(args, io.BytesIO(b""), out, err) == 2
    assert out.getvalue() == "" and "missing.txt" in err.getvalue()
    args = agrep_parser().parse_args(["-C", "-1", "needle", "1"])
    assert run_agrep(args, io.BytesIO(b""), io.StringIO(), io.StringIO()) == 2
