"""CPU checker for Searcher.search_all_alignments, written from its contract (include/sassy_hip.h; the reference's
src/search.rs:702-760 and src/alignment_iterator.rs:44-370) -- TEST INFRASTRUCTURE ONLY.

Two independent ways to the same set of alignments of one end position:

* ``dfs``: the contract's depth-first search from cell (end, m) of the DP matrix of the pattern against the text
  (top row 0, left column j), edges filtered by the rules with plain slice compares (no band, no run tables);
* ``brute``: every path from (end, m) to row 0 of cost <= k, with no pruning at all, filtered afterwards by the rules
  as predicates on the whole path.  The cost prune of the DFS never removes a complete path of cost <= k (the DP value
  of a cell is at most the cost of any path from it to row 0), so the two must agree as sets.

End positions come from the oracle (``oracle.search_modes(..., all_minima=True, without_trace=True)``), used
read-only.  Groups are returned in the contract's order as lists of tuples
(text_start, text_end, pattern_start, pattern_end, cost, strand, cigar).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

import oracle

# IUPAC letter (5 low bits) -> base set; 255 = not a letter (reference: src/profiles/iupac.rs:281-317)
_IUPAC = [255, 1, 14, 2, 13, 255, 255, 8, 7, 255, 255, 12, 255, 3, 15, 255,
          255, 255, 9, 10, 4, 4, 11, 5, 0, 6, 255, 255, 255, 255, 255, 255]


def scan_eq(profile: str, p: int, t: int) -> bool:
    """The equality of the DP costs (what the scan's profile encodes)."""
    if profile == "dna":
        return ((p >> 1) & 3) == ((t >> 1) & 3)
    if profile == "iupac":
        return (_IUPAC[p & 31] & _IUPAC[t & 31] & 15) != 0
    return p == t


def is_match(profile: str, p: int, t: int) -> bool:
    """Profile::is_match ('=' against 'X', and the diagonal rules' is_match_slice)."""
    if profile == "dna":
        return (p | 0x20) == (t | 0x20)
    if profile == "iupac":
        return (_IUPAC[p & 31] & _IUPAC[t & 31]) != 0
    return p == t


def rle(ops: List[str]) -> str:
    out, i = [], 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j] == ops[i]:
            j += 1
        out.append(f"{j - i}{ops[i]}")
        i = j
    return "".join(out)


def n_frac_ok(text: bytes, s: int, e: int, max_n_frac: float) -> bool:
    """src/n_filter.rs: check_n_fraction on the alignment's own span, in f32."""
    if s >= len(text) or e <= s:
        return True
    nn = sum(1 for c in text[s:e] if c | 0x20 == 0x6E)
    return bool(np.float32(nn) / np.float32(e - s) <= np.float32(max_n_frac))


def _fill(profile: str, pat: bytes, text: bytes, e: int, k: int):
    """DP over the window text[o .. e), o = e - (m + k) clipped at 0: D[i][0] = 0 for every column, D[o][j] = j."""
    m = len(pat)
    o = max(0, e - (m + k))
    W = e - o
    D = [[0] * (m + 1) for _ in range(W + 1)]
    for j in range(m + 1):
        D[0][j] = j
    for i in range(1, W + 1):
        t = text[o + i - 1]
        col, prev = D[i], D[i - 1]
        for j in range(1, m + 1):
            v = prev[j - 1] + (0 if scan_eq(profile, pat[j - 1], t) else 1)
            v = min(v, prev[j] + 1, col[j - 1] + 1)
            col[j] = v
    return o, D


def _net(ops: List[str]) -> int:
    """Net insertions since the last '=' of the ops taken so far (end -> start order)."""
    net = 0
    for op in reversed(ops):
        if op == "=":
            break
        if op == "I":
            net += 1
        elif op == "D":
            net -= 1
    return net


def _leave_blocked(profile, pat, text, i, j) -> bool:
    """At (i, j): the diagonal matches exactly all the way up to row 0."""
    ps, ts = pat[:j], text[max(i - j, 0):i]
    return len(ps) == len(ts) and all(is_match(profile, a, b) for a, b in zip(ps, ts))


def _enter_blocked(profile, pat, text, ni, nj, last) -> bool:
    """Entering (ni, nj): its diagonal matches exactly down to `last` (reads past the end position, up to len(text))."""
    ps = pat[nj:last]
    if ni + len(ps) > len(text):
        return False
    return all(is_match(profile, a, b) for a, b in zip(ps, text[ni:ni + len(ps)]))


def _diag(i, j) -> int:
    return i - j


def dfs_one_end(profile: str, pat: bytes, text: bytes, e: int, k: int) -> List[Tuple[int, int, str]]:
    """The contract's DFS at end position e: [(text_start, cost, cigar)] in visiting order."""
    m = len(pat)
    o, D = _fill(profile, pat, text, e, k)

    def cell(i, j):
        return D[i - o][j]

    if cell(e, m) > k:
        return []
    out = []
    last_row = {}
    ops: List[str] = []

    def visit(i, j, cost):
        if j == 0:
            out.append((i, cost, rle(ops[::-1])))
            return
        edges = []
        for op in ("M", "D", "I"):
            if op == "D" and (j == 0 or j == m):
                continue
            di, dj = {"M": (1, 1), "D": (1, 0), "I": (0, 1)}[op]
            if i < di or j < dj:
                continue
            ni, nj = i - di, j - dj
            if ni < o:
                continue
            name = op
            ec = 1
            if op == "M":
                name = "=" if is_match(profile, text[ni], pat[nj]) else "X"
                ec = 0 if name == "=" else 1
            total = cost + ec + cell(ni, nj)
            if total > k:
                continue
            if op in "ID":
                if _leave_blocked(profile, pat, text, i, j):
                    continue
                if _enter_blocked(profile, pat, text, ni, nj, last_row.get(_diag(ni, nj), m)):
                    continue
                net = _net(ops)
                if (op == "I" and net < 0) or (op == "D" and net > 0):
                    continue
            edges.append((name, total, ni, nj, ec))
        edges.sort(key=lambda x: x[1])  # stable: ties keep diagonal, D, I
        for name, _t, ni, nj, ec in edges:
            dg = _diag(ni, nj)
            old = last_row.get(dg)
            last_row[dg] = nj
            ops.append(name)
            visit(ni, nj, cost + ec)
            ops.pop()
            if old is None:
                del last_row[dg]
            else:
                last_row[dg] = old

    visit(e, m, 0)
    return out


def brute_one_end(profile: str, pat: bytes, text: bytes, e: int, k: int) -> List[Tuple[int, int, str]]:
    """Every path of cost <= k from (e, m) to row 0, then the rules as predicates on the path: a set."""
    m = len(pat)
    paths = []

    def walk(i, j, cost, steps):
        if j == 0:
            paths.append(list(steps))
            return
        for op, di, dj in (("M", 1, 1), ("D", 1, 0), ("I", 0, 1)):
            if i < di or j < dj:
                continue
            ni, nj = i - di, j - dj
            ec = 1
            name = op
            if op == "M":
                name = "=" if is_match(profile, text[ni], pat[nj]) else "X"
                ec = 0 if name == "=" else 1
            if cost + ec > k:
                continue
            steps.append((name, i, j, ni, nj))
            walk(ni, nj, cost + ec, steps)
            steps.pop()

    walk(e, m, 0, [])
    out = set()
    for steps in paths:
        names = [s[0] for s in steps]
        if names and (names[0] == "D" or names[-1] == "D"):
            continue
        ok = True
        last_row = {}
        for x, (name, i, j, ni, nj) in enumerate(steps):
            if name in "ID":
                if _leave_blocked(profile, pat, text, i, j):
                    ok = False
                if _enter_blocked(profile, pat, text, ni, nj, last_row.get(_diag(ni, nj), m)):
                    ok = False
                net = _net(names[:x])
                if (name == "I" and net < 0) or (name == "D" and net > 0):
                    ok = False
            if not ok:
                break
            last_row[_diag(ni, nj)] = nj
        if ok:
            cost = sum(0 if s[0] == "=" else 1 for s in steps)
            out.add((steps[-1][3] if steps else e, cost, rle(names[::-1])))
    return sorted(out)


def end_positions(profile: str, pattern: bytes, text: bytes, k: int, rc: bool,
                  max_n_frac: Optional[float] = None, only_best: bool = False) -> Tuple[List[int], List[int]]:
    """(Fwd ends ascending, Rc ends on the reversed text ascending) of search_all without trace."""
    ms = oracle.search_modes(profile, pattern, text, k, rc=rc, all_minima=True, max_n_frac=max_n_frac,
                             only_best=only_best, without_trace=True)
    n = len(text)
    fwd = sorted(x.text_end for x in ms if x.strand == "+")
    rev = sorted(n - x.text_start for x in ms if x.strand == "-")
    return fwd, rev


def search_all_alignments(profile: str, pattern: bytes, text: bytes, k: int, rc: bool = False,
                          max_n_frac: Optional[float] = None, only_best: bool = False, brute: bool = False):
    """The contract's groups, in its order.  brute=True: every group from brute_one_end (sorted inside a group)."""
    profile = profile.lower()
    pattern, text = bytes(pattern), bytes(text)
    n, m = len(text), len(pattern)
    nf = None if max_n_frac is None or max_n_frac == 1.0 else max_n_frac
    fwd, rev = end_positions(profile, pattern, text, k, rc, nf, only_best)
    one = brute_one_end if brute else dfs_one_end
    groups = []
    for e in fwd:
        g = [(s, e, 0, m, c, "+", cig) for (s, c, cig) in one(profile, pattern, text, e, k)]
        if nf is not None:
            g = [x for x in g if n_frac_ok(text, x[0], x[1], nf)]
        if g:
            groups.append(g)
    if rc:
        cp, rt = oracle.complement(profile, pattern), text[::-1]
        for e in rev:
            g = [(n - e, n - s, 0, m, c, "-", cig) for (s, c, cig) in one(profile, cp, rt, e, k)]
            if nf is not None:
                g = [x for x in g if n_frac_ok(text, x[0], x[1], nf)]
            if g:
                groups.append(g)
    return groups


def as_tuples(groups) -> list:
    """Library groups (lists of sassy_amd.Match) in the checker's tuple form."""
    return [[(x.text_start, x.text_end, x.pattern_start, x.pattern_end, x.cost, x.strand, x.cigar) for x in g]
            for g in groups]


def check_golden(entry: dict, groups) -> None:
    """The reference test's assertions (tests/golden/all_alignments.json) on groups of tuples."""
    ex = entry["expect"]
    flat = [x for g in groups for x in g]
    if "groups" in ex:
        assert len(groups) == ex["groups"], (entry["name"], groups)
    if "total" in ex:
        assert len(flat) == ex["total"], (entry["name"], len(flat))
    if "group_len_each" in ex:
        assert all(len(g) == ex["group_len_each"] for g in groups), (entry["name"], groups)
    if "text_ends" in ex:
        assert [g[0][1] for g in groups] == ex["text_ends"], (entry["name"], groups)
    if "nonempty" in ex:
        assert flat, entry["name"]
    for key, col in (("cost", 4), ("pattern_start", 2), ("pattern_end", 3), ("cigar", 6)):
        if key in ex.get("all", {}):
            assert all(x[col] == ex["all"][key] for x in flat), (entry["name"], key, flat)
    if "span" in ex.get("all", {}):
        assert all(x[1] - x[0] == ex["all"]["span"] for x in flat), (entry["name"], flat)
    if "first" in ex:
        f = groups[0][0]
        for key, col in (("text_start", 0), ("text_end", 1), ("pattern_start", 2), ("pattern_end", 3), ("cost", 4),
                         ("cigar", 6)):
            if key in ex["first"]:
                assert f[col] == ex["first"][key], (entry["name"], key, f)
    if "multi" in ex:
        multi = [g for g in groups if len(g) > 1]
        assert len(multi) == ex["multi"]["groups"], (entry["name"], groups)
        g = multi[0]
        assert len(g) == ex["multi"]["size"], (entry["name"], g)
        assert all(x[4] == ex["multi"]["cost"] and x[2] == 0 for x in g), (entry["name"], g)
        assert len({x[6] for x in g}) == ex["multi"]["distinct_cigars"], (entry["name"], g)
    if ex.get("no_edge_deletion"):
        for x in flat:
            # (as the reference: the first alphabetic character -- '=' is none -- and the last character)
            letters = [c for c in x[6] if c.isalpha()]
            assert (not letters or letters[0] != "D") and not x[6].endswith("D"), (entry["name"], x)
