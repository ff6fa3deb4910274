"""The definitions of include/sassy_hip.h: sassy_hip_LineSpan, restated with bytes.count / rfind / find.

'\\n' is the only separator.  For a position p of a text t of n bytes:
    line_no(p)    = 1 + the number of '\\n' in t[0:p]
    line_start(p) = 1 + the index of the last '\\n' in t[0:p], 0 if there is none
    line_end(p)   = the index of the first '\\n' in t[p:n], n if there is none
"""


def line_no(t: bytes, p: int) -> int:
    return 1 + t.count(b"\n", 0, p)


def line_start(t: bytes, p: int) -> int:
    return t.rfind(b"\n", 0, p) + 1


def line_end(t: bytes, p: int) -> int:
    e = t.find(b"\n", p)
    return len(t) if e < 0 else e


def line_span(t: bytes, first: int, last: int):
    """(line_no, last_line_no, line_start, line_end) of the span [first, last], first <= last <= len(t)."""
    assert 0 <= first <= last <= len(t)
    return line_no(t, first), line_no(t, last), line_start(t, first), line_end(t, last)


def match_span(t: bytes, text_start: int, text_end: int):
    """The span of a match [text_start, text_end): first = text_start, last = max(text_start, text_end - 1)."""
    return line_span(t, text_start, max(text_start, text_end - 1))


def line_spans(t: bytes, first, last):
    return [line_span(t, int(a), int(b)) for a, b in zip(first, last)]
