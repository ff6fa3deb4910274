"""Character-class patterns restated in numpy: the last DP row under "text byte is a member of the row's set", and a cigar
replayer for the records of Searcher.search_classes.

A pattern is a list of m sets of byte values (anything `in` works on: set, frozenset, bytes).  D[0][i] = 0, D[j][0] = j,
D[j][i] = min(D[j-1][i-1] + (text[i-1] not in set j), D[j-1][i] + 1, D[j][i-1] + 1); the last row is D[m][0 .. n].
"""
import re

import numpy as np


def member_table(sets):
    """(m, 256) bool: table[j][c] = byte value c is in set j."""
    tab = np.zeros((len(sets), 256), dtype=bool)
    for j, s in enumerate(sets):
        for c in s:
            tab[j, int(c)] = True
    return tab


def close_case(sets):
    """Every set closed under the A-Z / a-z twin (what an ascii_ci searcher does with a class pattern)."""
    out = []
    for s in sets:
        t = set(int(c) for c in s)
        for c in list(t):
            if 65 <= c <= 90 or 97 <= c <= 122:
                t.add(c ^ 0x20)
        out.append(frozenset(t))
    return out


def last_row(sets, text: bytes):
    """D[m][0 .. n] as int32, n = len(text)."""
    tab = member_table(sets)
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(t)
    idx = np.arange(n + 1, dtype=np.int32)
    prev = np.zeros(n + 1, dtype=np.int32)
    for j in range(len(sets)):
        miss = (~tab[j][t]).astype(np.int32)
        cur = np.empty(n + 1, dtype=np.int32)
        cur[0] = j + 1
        cur[1:] = np.minimum(prev[:-1] + miss, prev[1:] + 1)
        # the left neighbour: D[j][i] = min over i' <= i of (cur[i'] + i - i')
        cur = np.minimum.accumulate(cur - idx) + idx
        prev = cur
    return prev


_CIGAR = re.compile(r"(\d+)([=XID])")


def replay(sets, text: bytes, m) -> None:
    """Asserts that record `m` (text_start, text_end, pattern_start, pattern_end, cost, cigar) is an alignment of the
    whole pattern to text[text_start:text_end] under set membership: '=' columns are members, 'X' columns are not, 'D'
    consumes a text byte, 'I' a pattern row, and the cost is #X + #I + #D."""
    tab = member_table(sets)
    ops = _CIGAR.findall(m.cigar)
    assert "".join(a + b for a, b in ops) == m.cigar and m.cigar, m
    i, j, cost = m.text_start, 0, 0
    for cnt, op in ops:
        for _ in range(int(cnt)):
            if op in "=X":
                assert i < m.text_end and j < len(sets), m
                assert bool(tab[j, text[i]]) == (op == "="), (m, i, j)
                i += 1
                j += 1
            elif op == "D":
                assert i < m.text_end, m
                i += 1
            else:
                assert j < len(sets), m
                j += 1
            cost += op != "="
    assert j == len(sets) and (m.pattern_start, m.pattern_end) == (0, len(sets)), m
    assert i == m.text_end, m
    assert cost == m.cost, (m, cost)
