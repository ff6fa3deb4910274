"""Shapes and texts for the grouped and kept-plane text passes (pure Python and the oracle, no device): member pairs of
every piece length Q = 7 .. 12 the launches are instantiated for, with unequal piece counts, rows behind the last piece,
and lone shapes of 8 pieces -- and per pair one text made of the prefilter adversary's layouts
(tests/helpers/filter_adversary.py), member A's followed by member B's, so that a piece slot given to the wrong member,
a wrong shift distance or a wrong row index loses a copy whose only intact piece is that slot.

Shared by tests/test_pass_shapes_cpu.py (the texts against the oracle: they are not vacuous) and
tests/test_gpu_pass_shapes.py (streams of searches in flight on them)."""
import collections
import random

import filter_adversary as fa

WORKGROUP = 4 * fa.BLOCK * fa.BLOCK * 8   # bytes of text per workgroup at 8 blocks per lane chunk: 4 waves of 64 lanes
ODD_CUT = 37                              # the second text of a pair: the first less its last 37 bytes, an odd length

# offset: added to the pattern's seed 1000 m + k (the seed of filter_adversary.shape_pattern)
Member = collections.namedtuple("Member", "m k offset")
# lone: b is a second pattern of a's shape (2 x 8 pieces never share a launch); the text is a's layout alone
Row = collections.namedtuple("Row", "q a b lone")
Joined = collections.namedtuple("Joined", "text odd pats ks copies starts")


def M(m, k, offset=0):
    return Member(m, k, offset)


def piece_len(m, k):
    """csrc/scan_route.h: filter_piece_len"""
    return min(m // (k + 1), 12)


def n_pieces(member):
    return member.k + 1


PAIRS = [
    Row(7, M(29, 3), M(21, 2), False),     # 4 + 3 pieces, one row behind A's last piece
    Row(7, M(35, 4), M(14, 1), False),     # 5 + 2
    Row(7, M(56, 7), M(56, 7, 2), True),   # 8 pieces, lone (seed offset 1 loses a class to the screen)
    Row(8, M(32, 3), M(32, 3, 1), False),  # 4 + 4: the shape of every earlier pass test, two patterns
    Row(8, M(40, 4), M(24, 2), False),     # 5 + 3
    Row(8, M(56, 6, 7919), M(56, 6, 7920), True),   # 7 pieces in the eight-slot kernel, lone
    Row(9, M(37, 3), M(18, 1), False),     # 4 + 2, one row behind
    Row(9, M(36, 3), M(27, 2), False),     # 4 + 3
    Row(10, M(43, 3), M(30, 2), False),    # 4 + 3, three rows behind
    Row(10, M(40, 3), M(20, 1), False),    # 4 + 2
    Row(11, M(47, 3), M(22, 1), False),    # 4 + 2, three rows behind
    Row(11, M(44, 3), M(33, 2), False),    # 4 + 3
    Row(12, M(128, 3), M(36, 2), False),   # 4 + 3, Q capped: 80 rows behind A's last piece, four pattern words
    Row(12, M(64, 3), M(48, 3), False),    # 4 + 4, 16 rows behind
    Row(12, M(100, 7), M(100, 7, 1), True),  # 8 pieces, lone, 4 rows behind
]
MIXED = [M(29, 3), M(32, 3), M(40, 3), M(48, 3)]   # Q = 7, 8, 10, 12: no two fit one launch, all share one plane key
MIXED_TWIN = M(40, 3, 1)                           # a second Q = 10 pattern, in the place of (32, 3)


def row_id(row):
    a, b = row.a, row.b
    return f"q{row.q}-lone-m{a.m}k{a.k}" if row.lone else f"q{row.q}-m{a.m}k{a.k}-m{b.m}k{b.k}"


def members():
    """Every member of PAIRS and of the mixed text, once."""
    out = []
    for row in PAIRS:
        out += [row.a, row.b]
    out += MIXED + [MIXED_TWIN]
    return list(dict.fromkeys(out))


def pattern(member):
    return fa.adversary_pattern(random.Random(1000 * member.m + member.k + member.offset), member.m)


_screened = {}


def screened(member):
    """(pattern, kept, dropped): the member's pigeonhole variants for its pieces through the oracle, once per process."""
    if member not in _screened:
        import oracle
        pat = pattern(member)
        variants = fa.variants_for(pat, member.k, ("pieces", piece_len(member.m, member.k)))
        _screened[member] = (pat,) + tuple(fa.screen(oracle.search, "dna", pat, member.k, variants, random.Random(5)))
    return _screened[member]


def join(laid):
    """One text of the layouts of `laid` (members), one behind the other.  Every layout is a multiple of 64 bytes, so block
    offsets survive the join; every layout's `must` columns are those of the whole text (filter_adversary.must_borders),
    shifted by what lies in front of it: its copies straddle the real lane, wave and workgroup borders.  copies[i]: member
    i's copies at their offsets in the whole text."""
    whole = fa.must_borders(len(laid) * (fa.MIN_BYTES + 4096))
    text, copies, starts = b"", [], []
    for mem in laid:
        pat, kept, _ = screened(mem)
        at = len(text)
        part, cs = fa.lay_out(kept, random.Random(100 * mem.m + mem.k + mem.offset), fa.MIN_BYTES, pat, mem.k, extra=0,
                              must=[x - at for x in whole if x > at])
        assert len(part) % fa.BLOCK == 0
        starts.append(at)
        copies.append([c._replace(start=c.start + at, end=c.end + at) for c in cs])
        text += part
    return text, copies, starts


_texts = {}


def _joined(searched, laid):
    kk = (tuple(searched), tuple(laid))
    if kk not in _texts:
        text, copies, starts = join(laid)
        _texts[kk] = Joined(text, text[:-ODD_CUT], [pattern(x) for x in searched], [x.k for x in searched], copies, starts)
    return _texts[kk]


def pair_text(a, b, lone=False):
    """Joined: the pair's text (a's layout, then b's; a lone shape: a's alone), the same text less its last ODD_CUT bytes
    (an odd length: the last wave's last blocks are not whole), both patterns and ks, the copies per laid-out member."""
    return _joined([a, b], [a] if lone else [a, b])


def row_text(row):
    return pair_text(row.a, row.b, row.lone)


def mixed_text(shapes, laid=None):
    """The same for members of different piece lengths: one layout each (laid: the members whose layouts make the text,
    where they are not the searched ones)."""
    return _joined(shapes, shapes if laid is None else laid)


def grid_of(n_bytes):
    """Workgroups of the pass over a whole text this short (8 blocks per lane chunk), and where its second half begins."""
    fgrid = (n_bytes + WORKGROUP - 1) // WORKGROUP
    return fgrid, (fgrid + 1) // 2 * WORKGROUP
