"""A deterministic adversary for the prefilters (pure Python, no device): planted copies of a pattern, each within k edits,
built against a given filter geometry so that the filter's bounds are met exactly -- every pigeonhole piece but one
destroyed, all k edits insertions (or all deletions) on one side of the survivor, a match end rem +- k columns from the
piece -- and a layout that puts those ends on both sides of block, lane, wave and workgroup borders.

Shared by tests/test_filter_adversary_cpu.py (the adversary against the oracle: it is not vacuous) and
tests/test_gpu_filter_adversary.py (every filter route against the oracle on the adversary's texts).

A row edit is (op, side): op 'S' substitutes the row's letter, 'D' leaves the row without a text character, 'I' keeps the
row and adds a text character in front of it (side 'front') or behind it (side 'behind').  A substituted or inserted
letter differs from the row and from both neighbouring rows, so no cheaper alignment takes it for one of them."""
import collections

BLOCK = 64
RUN_MERGE_GAP = 32            # scan_kernel.hip: kRunMergeGap -- runs of end columns this close share a window
END_OFFSETS = (62, 63, 0, 1)  # a copy's last byte within its 64-byte block: both sides of a border, both parities
KINDS = ("sub", "ins", "del", "alt")
MIN_BYTES = 160 * 1024 + 77   # past the first workgroup border of the smallest lane chunk (4 * 64 * 64 * 8 = 128 KiB)

Variant = collections.namedtuple("Variant", "data tag length row_at intact")
Copy = collections.namedtuple("Copy", "start end tag gap rc index")


_TO_BASE = bytes(b"ACGT"[i & 3] for i in range(256))

# (m, k): filter family.  The shapes tests/helpers/scan_routes.py names per family, and the windows of the counting
# filter on either side of a 64 multiple.
SHAPES = {
    (12, 1): "short", (18, 2): "short", (24, 3): "short",
    (23, 3): "paired", (32, 4): "paired", (32, 5): "paired",
    (20, 2): "counting", (27, 3): "counting", (33, 3): "counting", (69, 1): "counting", (70, 1): "counting",
    (32, 3): "planes", (40, 2): "planes", (64, 3): "planes", (65, 3): "planes", (100, 5): "planes",
    (100, 9): "table", (300, 8): "table",
}


def shape_pattern(m, k):
    """The shape's pattern.  Its seed is one for which the oracle keeps every (survivor, kind, layout) class and at least
    98 % of the shape's variants (test_filter_adversary_cpu.py asserts both); a shape that misses takes another seed."""
    import random
    return adversary_pattern(random.Random(1000 * m + k), m)


def shape_geometries(m, k):
    """geometries() and the many-pattern filter's where it takes the shape (<= 8 pieces of >= 6 rows)."""
    return geometries(m, k) + ([("multi", min(m // (k + 1), 12))] if k + 1 <= 8 and m // (k + 1) >= 6 else [])


def adversary_pattern(rng, m):
    """m random bases, no two neighbours equal: deleting a row next to a piece then never restores the piece."""
    p = bytearray()
    while len(p) < m:
        c = rng.choice(b"ACGT")
        if not p or p[-1] != c:
            p.append(c)
    return bytes(p)


def _other(pat, i):
    """A base that differs from row i and from both of its neighbours (the choice rotates with i)."""
    near = {pat[j] for j in (i - 1, i, i + 1) if 0 <= j < len(pat)}
    free = [c for c in b"ACGT" if c not in near] or [c for c in b"ACGT" if c != pat[i]]
    return free[i % len(free)]


def apply_edits(pat, edits, wild=()):
    """(bytes, row_at): the pattern with `edits` = {row: (op, side)} applied; row_at[i] = the text offset that holds row i
    unchanged, -1 for a substituted or deleted row.  wild: rows that accept any letter (an N of the searched pattern) --
    a substitution there is no edit, and edits that hold one give (None, None): no variant."""
    if any(op == "S" and r in wild for r, (op, _) in edits.items()):
        return None, None
    out, row_at = bytearray(), []
    for i, c in enumerate(pat):
        op, side = edits.get(i, (None, None))
        if op == "S":
            out.append(_other(pat, i))
            row_at.append(-1)
        elif op == "D":
            row_at.append(-1)
        elif op == "I" and side == "front":
            out.append(_other(pat, i))
            row_at.append(len(out))
            out.append(c)
        elif op == "I":
            row_at.append(len(out))
            out.append(c)
            out.append(_other(pat, i))
        else:
            assert op is None, op
            row_at.append(len(out))
            out.append(c)
    return bytes(out), row_at


def _ops(kind, n):
    return {"sub": "S" * n, "ins": "I" * n, "del": "D" * n, "alt": ("ID" * n)[:n]}[kind]


def _variant(pat, rows, kind, side_of, tag, wild=()):
    rows = sorted(rows)
    edits = {r: (op, side_of(r)) for r, op in zip(rows, _ops(kind, len(rows)))}
    data, row_at = apply_edits(pat, edits, wild)
    return Variant(data, tag, len(data), row_at, None) if data is not None else None


def _anchored(rows, m, k):
    """A run of edits in neighbouring rows needs more than k intact rows on either side -- k + 1 and a quarter more, since
    random filler matches one row in four: the ends of a match are free, so the oracle gives up a shorter end of the pattern
    for less than the run costs, and the copy is no longer at k."""
    need = k + 1 + (k + 3) // 4
    return min(rows) >= need and m - 1 - max(rows) >= need


def piece_bounds(q, n_pieces):
    return [(p * q, (p + 1) * q) for p in range(n_pieces)]


def pigeonhole_variants(pat, k, q, n_pieces, bounds=None, wild=()):
    """Copies of `pat` with exactly k edits against n_pieces = k + 1 pigeonhole pieces (piece p = rows [p q, (p+1) q); the
    rows behind the last piece belong to none; `bounds`: other [first, last) rows per piece), tagged (survivor, kind, layout):
      'mid'     one edit in the middle row of every destroyed piece;
      'border'  one edit in every destroyed piece, in its row nearest to the survivor: the rows directly next to the
                survivor are edited, its own rows stay;
      'behind'  all k edits in the rows directly behind the survivor where there is room (every second row for 'sub' and
                'alt': substitutions in a row, or an insertion next to a deletion, align cheaper), no other piece
                edited: the match ends rem + k (all insertions) or rem - k (all deletions) columns behind the piece;
      'front'   the mirror: all k in the rows directly in front of the survivor, the longest and shortest span in front.
    'behind' and 'front' exist where the run of edits keeps more than k intact rows on either side (_anchored).
    With 'mid' and 'border' the survivor is the only intact piece; with 'behind' / 'front' the pieces on the unedited side
    survive as well, and the survivor is the only one for piece 0 / the last piece where k edits reach every other piece."""
    m = len(pat)
    bounds = bounds or piece_bounds(q, n_pieces)
    assert len(bounds) == n_pieces == k + 1 and bounds[-1][1] <= m, (m, k, q, n_pieces)
    out = []
    for p, (s_p, e_p) in enumerate(bounds):
        # an inserted character lies on the side of its row that is away from the survivor: inside the row's piece
        inside = lambda r: "front" if r < s_p else "behind"
        for kind in KINDS:
            step = 1 if kind in ("ins", "del") else 2
            layouts = {
                "mid": [s + (e - s) // 2 for u, (s, e) in enumerate(bounds) if u != p],
                "border": [e - 1 if u < p else s for u, (s, e) in enumerate(bounds) if u != p],
                "behind": [e_p + step * i for i in range(k)],
                "front": [s_p - 1 - step * i for i in range(k)],
            }
            for layout, rows in layouts.items():
                if not rows or min(rows) < 0 or max(rows) >= m:
                    continue  # no room on that side of the survivor
                if layout in ("behind", "front") and not _anchored(rows, m, k):
                    continue
                out.append(_variant(pat, rows, kind, inside, (p, kind, layout), wild))
    return [v for v in out if v is not None]


def pair_geometry(m, k):
    """(S, Q) of the paired filter -- S = ceil((k+1)/2) super-pieces of two sub-pieces of Q = m / (2 S) rows -- or None
    where the shape is not one of its (csrc/scan_route.h: pair_geometry)."""
    if k < 1 or m // (k + 1) >= 7:
        return None
    s = (k + 2) // 2
    q = m // (2 * s)
    return (s, q) if s <= 4 and q in (5, 6) else None


def pair_variants(pat, k, S, Q, wild=()):
    """Copies with exactly k edits against the paired filter's pigeonhole: super-piece t keeps ONE edit -- every row of both
    of its halves, kinds sub / ins / del -- tagged (t, kind, layout):
      'far'     the other super-pieces take two substitutions each while the budget lasts, away from their borders;
      'behind'  the rest of the budget in the rows directly behind super-piece t, as insertions (the single edit an
                insertion, or a substitution in an even row) or as deletions: same-direction indels next to the survivor;
      'front'   the mirror, in the rows directly in front of it."""
    m = len(pat)
    assert 2 * S * Q <= m
    out = []
    for t in range(S):
        lo, hi = t * 2 * Q, (t + 1) * 2 * Q
        for j in range(2 * Q):
            for kind in ("sub", "ins", "del"):
                if kind == "ins" and lo + j == 0:
                    continue  # a character in front of row 0 is filler, not an edit
                one = {lo + j: ({"sub": "S", "ins": "I", "del": "D"}[kind], "front")}
                far, budget = dict(one), k - 1
                for u in range(S):
                    for off in (1, Q + 1):
                        if u != t and budget > 0:
                            far[u * 2 * Q + off] = ("S", None)
                            budget -= 1
                layouts = {"far": far}
                if k > 1:
                    op = "I" if kind == "ins" or (kind == "sub" and j % 2 == 0) else "D"
                    if _anchored([lo + j, hi + k - 2], m, k):
                        layouts["behind"] = {**one, **{hi + i: (op, "front") for i in range(k - 1)}}
                    if _anchored([lo - (k - 1), lo + j], m, k):
                        layouts["front"] = {**one, **{lo - 1 - i: (op, "behind") for i in range(k - 1)}}
                for layout, edits in layouts.items():
                    data, row_at = apply_edits(pat, edits, wild)
                    if data is not None:
                        out.append(Variant(data, (t, kind, layout), len(data), row_at, None))
    return out


def qgram_threshold(m, k, Q):
    """The counting filter's threshold (q-gram lemma): a match within k edits keeps at least this many of the m - Q + 1."""
    return m + 1 - (k + 1) * Q


def qgram_variants(pat, k, Q, wild=()):
    """Copies with exactly k edits at rows r, r + Q, ... for every phase r in 0 .. Q-1 and every kind, tagged (r, kind,
    'phase'); `intact` = how many of the pattern's Q-grams no edit touches (a substituted or deleted row i takes the Q-grams
    that start in [i - Q + 1, i], a character inserted behind it those in [i - Q + 2, i])."""
    m = len(pat)
    assert (k + 1) * Q <= m
    out = []
    for r in range(Q):
        for kind in KINDS:
            rows = [r + Q * i for i in range(k)]
            gone = set()
            for row, op in zip(rows, _ops(kind, k)):
                gone.update(o for o in range(row - Q + (2 if op == "I" else 1), row + 1) if 0 <= o <= m - Q)
            v = _variant(pat, rows, kind, lambda r_: "behind", (r, kind, "phase"), wild)
            if v is not None:
                out.append(v._replace(intact=m - Q + 1 - len(gone)))
    return out


def geometries(m, k):
    """Every filter geometry a route may give the shape: ('pieces', q) for k + 1 pigeonhole pieces (the bit planes take up
    to 12 rows a piece, the q-gram table 9), ('pair', S, Q), ('qgram', Q) for the counting filter's variants."""
    out = []
    q0 = min(m // (k + 1), 12)
    for q in sorted({q0, min(q0, 9)}):
        if q >= 2:
            out.append(("pieces", q))
    if pair_geometry(m, k):
        out.append(("pair",) + pair_geometry(m, k))
    for Q in (5, 6, 7):
        if (k + 1) * Q <= m and (m + k - Q + 63) // 64 + 1 <= 64:
            out.append(("qgram", Q))
    return out


def variants_for(pat, k, geometry, wild=()):
    if geometry[0] == "pieces":
        return pigeonhole_variants(pat, k, geometry[1], k + 1, wild=wild)
    if geometry[0] == "pair":
        return pair_variants(pat, k, geometry[1], geometry[2], wild)
    if geometry[0] == "multi":  # filter_dna_multi_kernel: the first m mod (k+1) pieces one row longer
        return pigeonhole_variants(pat, k, geometry[1], k + 1, bounds=multi_bounds(len(pat), k), wild=wild)
    assert geometry[0] == "qgram", geometry
    return qgram_variants(pat, k, geometry[1], wild)


def multi_bounds(m, k):
    """The many-pattern filter's pieces (c_abi.hip: search_encoded): q = min(m / (k+1), 12) rows, + 1 for the first spare ones."""
    q = min(m // (k + 1), 12)
    spare = m - q * (k + 1)
    starts = [p * q + min(p, spare) for p in range(k + 1)]
    return [(s, s + q + (1 if p < spare else 0)) for p, s in enumerate(starts)]


def must_borders(n_bytes):
    """Columns some copy has to straddle: every wave border (64 lanes of bpl blocks) of every even bpl in 8 .. 32, the
    first workgroup border (4 waves) of bpl = 8, and 24 lane borders of every bpl, spread over the text."""
    xs = {4 * BLOCK * BLOCK * 8}
    for bpl in range(8, 33, 2):
        xs.update(range(BLOCK * BLOCK * bpl, n_bytes, BLOCK * BLOCK * bpl))
        lanes = range(BLOCK * bpl, n_bytes, BLOCK * bpl)
        xs.update(lanes[(2 * j + 1) * len(lanes) // 48] for j in range(24))
    return sorted(x for x in xs if x < n_bytes)


def straddles(copy, unit):
    """Does the copy have bytes on both sides of a multiple of `unit`?"""
    return (copy.start // unit + 1) * unit < copy.end


def lay_out(variants, rng, min_bytes, pat, k, extra=0, rc=None, must=None):
    """(text, copies): the variants between random ACGT filler, cycled (every pass shifts the offsets by one) until the text
    holds every variant and at least min_bytes.
      - a copy's last byte lies at offset 62, 63, 0, 1 of its block, in turn (a reverse-complemented copy: its first byte at
        1, 0, 63, 62 -- the match end as its strand reads it);
      - the filler in front of a copy is in turn short (< RUN_MERGE_GAP columns: the runs merge; taken where it reaches
        the copy's offset) and long (> m + k + 64: the window stands alone);
      - the copy that would pass a column of `must` is moved to straddle it;
      - the text begins with the pattern less its first j0 <= k rows and ends with it less its last j1 <= k rows;
      - its length is a multiple of 64, plus `extra`.
    rc: a function that reverse-complements a copy; it is applied to half of the plants."""
    m = len(pat)
    long_min = m + k + BLOCK + 1
    must = must_borders(min_bytes) if must is None else sorted(must)
    comp = (lambda c: rc(bytes([c]))[0]) if rc is not None else None
    head_of = lambda is_rc: {comp(pat[-1]), comp(pat[-2])} if is_rc else {pat[0], pat[1]}   # what continues a copy leftwards
    tail_of = lambda is_rc: {comp(pat[0]), comp(pat[1])} if is_rc else {pat[-1], pat[-2]}   # ... and rightwards
    j0 = k if extra == 0 else rng.randrange(k + 1)
    text = bytearray(pat[j0:])
    copies = [Copy(0, len(text), ("head", j0, None), 0, False, -1)]
    after = tail_of(False)
    i = mi = 0
    while len(text) < min_bytes or i < len(variants):
        idx, turn = i % len(variants), i // len(variants)
        v = variants[idx]
        data, is_rc = v.data, False
        if rc is not None and rng.random() < 0.5:
            data, is_rc = rc(data), True
        L, pos = len(data), len(text)
        o = END_OFFSETS[(idx + turn) % 4]
        g = (((BLOCK - 1 - o) if is_rc else (o + 1 - L)) - pos) % BLOCK
        if (idx + turn // 4) % 2 == 1:
            gap = g if g < RUN_MERGE_GAP else rng.randrange(1, RUN_MERGE_GAP)  # (out of reach: short, at any offset)
        else:
            gap = g + BLOCK * (max(0, long_min - g + BLOCK - 1) // BLOCK + rng.randrange(3))
        while mi < len(must):
            x = must[mi]
            if pos + gap + L <= x - (m + k + 2):
                break       # the next copy still fits in front of it
            forced = x + (o & 1) + 1 - L
            mi += 1
            if forced >= pos and L >= 3:
                gap = forced - pos
                break
        text += filler(rng, gap, after, head_of(is_rc)) + data
        after = tail_of(is_rc)
        copies.append(Copy(pos + gap, pos + gap + L, v.tag, gap, is_rc, idx))
        i += 1
    pos = len(text)
    n = (pos + long_min + m + BLOCK - 1) // BLOCK * BLOCK + extra
    j1 = k if extra == 0 else rng.randrange(k + 1)
    text += filler(rng, n - (m - j1) - pos, after, head_of(False)) + pat[:m - j1]
    copies.append(Copy(n - (m - j1), n, ("tail", j1, None), n - (m - j1) - pos, False, -1))
    assert len(text) == n
    return bytes(text), copies


def filler(rng, n, not_first=(), not_last=()):
    """n random bases; the first is none of `not_first` and the last none of `not_last` where a base is left: filler that
    does not continue the copy next to it (a deleted first row would come back for free)."""
    out = bytearray(rng.randbytes(n).translate(_TO_BASE))
    if n:
        out[0] = rng.choice([c for c in b"ACGT" if c not in not_first] or list(b"ACGT"))
        both = set(not_last) | (set(not_first) if n == 1 else set())
        out[-1] = rng.choice([c for c in b"ACGT" if c not in both] or [c for c in b"ACGT" if c not in not_last] or list(b"ACGT"))
    return bytes(out)


def screen(oracle_search, profile, pat, k, variants, rng, margin=100):
    """(kept, dropped): every variant alone between `margin` bytes of filler through the oracle -- kept where the matches
    that overlap the copy hold one of cost exactly k and none cheaper (the copy is as far from the pattern as it claims)."""
    kept, dropped = [], []
    for v in variants:
        text = filler(rng, margin, (), pat[:2]) + v.data + filler(rng, margin, pat[-2:], ())
        costs = [x.cost for x in oracle_search(profile, pat, text, k, all_minima=True)
                 if x.text_start < margin + v.length and x.text_end > margin]
        (kept if costs and min(costs) == k else dropped).append(v)
    return kept, dropped
