"""The texts of tests/helpers/piece_pair_texts.py hold what they claim (no device): every copy is in the text, its named slot
is its only intact piece, the piece lies where its kind says -- across the border in front of an even or an odd block, or
wholly in a block next to the other member's -- the oracle finds every copy within k, and no class (member x slot x kind)
is left without a copy by the oracle's screen.  The GPU tests on these texts: tests/test_gpu_piece_pair.py."""
import collections
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import filter_adversary as fa  # noqa: E402
import pass_shapes as ps  # noqa: E402
import piece_pair_texts as pt  # noqa: E402


@pytest.fixture(scope="module")
def oracle():
    sys.path.insert(0, ROOT)
    import oracle
    oracle.build()
    return oracle


@pytest.mark.parametrize("row", pt.ROWS + pt.HALO_ROWS[2:], ids=ps.row_id)
def test_every_copy_is_where_its_kind_says(oracle, row):
    T = pt.pair_text(row)
    members = (row.a, row.b)
    n = len(T.text)
    assert n >= fa.MIN_BYTES and n % (2 * fa.BLOCK) == 0 and len(T.odd) == n - ps.ODD_CUT and len(T.odd_blocks) == n - fa.BLOCK
    assert (len(T.odd_blocks) // fa.BLOCK) % 2 == 1
    classes = collections.Counter()
    for i, c in enumerate(T.plants):
        mem, q = members[c.member], row.q
        pat = T.pats[c.member]
        assert T.text[c.start:c.end] == c.data and (i == 0 or c.start >= T.plants[i - 1].end + 2), c
        # the named slot is intact, every other piece of the member is nowhere in the copy
        assert T.text[c.lo:c.hi] == pat[c.slot * q:(c.slot + 1) * q] and c.hi - c.lo == q, c
        for u in range(ps.n_pieces(mem)):
            assert (pat[u * q:(u + 1) * q] in c.data) == (u == c.slot), (c, u)
        first, last = c.lo // fa.BLOCK, (c.hi - 1) // fa.BLOCK
        if c.kind in ("even", "odd"):
            assert last == first + 1 and last % 2 == (c.kind == "odd"), c
        elif c.kind == "first":
            o = T.plants[i + 1]
            assert first == last and o.kind == "second" and o.member != c.member, (c, o)
            assert o.lo // fa.BLOCK == (o.hi - 1) // fa.BLOCK == first + 1, (c, o)
        elif c.kind == "second":
            assert first == last and T.plants[i - 1].kind == "first", c
        else:
            assert c.kind == "last", c
        classes[(c.member, c.slot, c.kind)] += 1
    # both parities of the first block of a neighbouring pair
    firsts = collections.Counter((c.member, c.slot, (c.lo // fa.BLOCK) & 1) for c in T.plants if c.kind == "first")
    seconds = collections.Counter((c.member, c.slot) for c in T.plants if c.kind == "second")
    for mi, mem in enumerate(members):
        for slot in range(ps.n_pieces(mem)):
            gen, gone = T.generated[mi][slot], T.dropped[mi][slot]
            print(f"{ps.row_id(row)} member {mi} slot {slot}: generated {gen} dropped {gone} | " +
                  " ".join(f"{kind} {classes[(mi, slot, kind)]}" for kind in pt.KINDS))
            assert gen > gone, (mi, slot)
            for kind in pt.KINDS[:3]:
                assert classes[(mi, slot, kind)] >= 1, (mi, slot, kind)
            assert firsts[(mi, slot, 0)] >= 1 and firsts[(mi, slot, 1)] >= 1 and seconds[(mi, slot)] >= 1, (mi, slot)
    # copies behind the first workgroup border, and in the last block of the text and of the text less a block
    assert max(c.start for c in T.plants if c.kind != "last") > ps.WORKGROUP
    ends = [c.end for c in T.plants if c.kind == "last"]
    assert [(e - 1) // fa.BLOCK for e in ends] == [n // fa.BLOCK - 2, n // fa.BLOCK - 1]
    # not vacuous: the oracle reports a match within k over every copy
    for mi in (0, 1):
        found = sorted((x.text_start, x.text_end) for x in oracle.search("dna", T.pats[mi], T.text, T.ks[mi]))
        assert len(found) >= sum(1 for c in T.plants if c.member == mi)
        j = 0
        for c in (c for c in T.plants if c.member == mi):
            while j < len(found) and found[j][1] <= c.lo:
                j += 1
            assert j < len(found) and found[j][0] < c.hi, (mi, c)


def test_dense_text_fills_the_queues():
    row = pt.ROWS[1]
    text, pats, ks = pt.dense_text(row)
    assert len(text) >= 3 * ps.WORKGROUP and (row.a, row.b) == (ps.M(32, 3), ps.M(32, 3, 1))
    wave = fa.BLOCK * fa.BLOCK * 8  # bytes a wave streams at 8 blocks per lane chunk
    for w in range(len(text) // wave):
        for j, p in enumerate(pats):  # 128 windows per wave and member: twice fuse_press = 64
            assert sum(text[at:at + len(p)] == p for at in range(w * wave + 128 * j, (w + 1) * wave - 256, 256)) >= 126
