"""CPU-only: the texts of tests/helpers/pass_shapes.py against the oracle -- they are not vacuous.  Per shape the condition
of test_filter_adversary_cpu.py (at most 2 % of the variants leave, no (survivor, kind, layout) class is lost); per pair
every piece slot of either member is the sole survivor of a copy in the text, copies of each member lie on both sides of
a lane, a wave and a workgroup border and one ends at the border between the pass's two halves, and the two members'
matches differ -- so a launch that hands a slot to the wrong member, or a member's reports to the other, loses records."""
import os
import random
import sys
import time

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import filter_adversary as fa  # noqa: E402
import pass_shapes as ps  # noqa: E402
import oracle  # noqa: E402

MEMBERS = ps.members()
mem_id = lambda x: f"m{x.m}k{x.k}" + (f"s{x.offset}" if x.offset else "")


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle.build()


def test_table_is_what_the_launches_take():
    """Both members of a pair have the row's piece length (7 .. 12, every one of them), at most 8 pieces together and
    patterns of at most four words; a lone shape has more than 4 pieces (two of them never share a launch); the pairs hold
    unequal piece counts, and shapes with rows behind the last piece."""
    assert {row.q for row in ps.PAIRS} == set(range(7, 13))
    for row in ps.PAIRS:
        for x in (row.a, row.b):
            assert ps.piece_len(x.m, x.k) == row.q and x.m // (x.k + 1) >= 7 and x.m <= 128, row
        if row.lone:
            assert (row.a.m, row.a.k) == (row.b.m, row.b.k) and 5 <= ps.n_pieces(row.a) <= 8
            assert ps.pattern(row.a) != ps.pattern(row.b)
        else:
            assert ps.n_pieces(row.a) + ps.n_pieces(row.b) <= 8, row
    counts = {(ps.n_pieces(r.a), ps.n_pieces(r.b)) for r in ps.PAIRS if not r.lone}
    assert counts >= {(4, 3), (5, 2), (5, 3), (4, 4), (4, 2)}
    assert {ps.n_pieces(r.a) for r in ps.PAIRS if r.lone} == {7, 8}
    for q in range(7, 13):  # rows behind the last piece at every piece length but 8 (m = 8 (k+1) in both of its pairs)
        behind = [x.m - q * (x.k + 1) for r in ps.PAIRS if r.q == q and not r.lone for x in (r.a, r.b)]
        assert q == 8 or max(behind) > 0, (q, behind)
    assert sorted(ps.piece_len(x.m, x.k) for x in ps.MIXED) == [7, 8, 10, 12]
    assert ps.piece_len(ps.MIXED_TWIN.m, ps.MIXED_TWIN.k) == 10 and ps.pattern(ps.MIXED_TWIN) != ps.pattern(ps.M(40, 3))


@pytest.mark.parametrize("member", MEMBERS, ids=mem_id)
def test_oracle_agreement(member):
    """Alone in filler, every variant has an oracle match over it of cost exactly k and none cheaper; at most 2 % of a
    shape's variants miss that, and every (survivor, kind, layout) class keeps a variant."""
    pat, kept, dropped = ps.screened(member)
    total = len(kept) + len(dropped)
    lost = {v.tag for v in dropped} - {v.tag for v in kept}
    assert not lost, (member, sorted(lost))
    assert {v.tag[0] for v in kept} == set(range(member.k + 1))
    assert {v.tag[1] for v in kept} == set(fa.KINDS) and {v.tag[2] for v in kept} >= {"mid", "border"}
    print(f"shape {mem_id(member)}: Q {ps.piece_len(member.m, member.k)}, variants {total}, dropped {len(dropped)}")
    assert len(dropped) * 50 <= total, (member, len(dropped), total)


def _sole_survivors(text, copies, pat, k, q):
    """The slots p for which some 'mid' / 'border' copy in the text holds piece p's rows and the rows of no other piece
    (but for pieces the pattern itself repeats)."""
    bounds = fa.piece_bounds(q, k + 1)
    twice = {u for u, (s, e) in enumerate(bounds) if pat.find(pat[s:e], pat.find(pat[s:e]) + 1) >= 0}
    out = set()
    for c in copies:
        if c.index < 0 or c.tag[2] not in ("mid", "border"):
            continue
        data = text[c.start:c.end]
        found = [u for u, (s, e) in enumerate(bounds) if data.find(pat[s:e]) >= 0]
        if c.tag[0] in found and [u for u in found if u == c.tag[0] or u not in twice] == [c.tag[0]]:
            out.add(c.tag[0])
    return out


@pytest.mark.parametrize("row", ps.PAIRS, ids=ps.row_id)
def test_pair_text(row):
    J = ps.row_text(row)
    n = len(J.text)
    laid = [row.a] if row.lone else [row.a, row.b]
    assert n % 64 == 0 and len(J.odd) == n - ps.ODD_CUT and len(J.odd) % 2 == 1 and n < (1 << 20)
    assert set(J.text) <= set(b"ACGT")
    fgrid, half = ps.grid_of(n)
    assert ps.grid_of(len(J.odd)) == (fgrid, half)
    assert (fgrid, half) == ((2, ps.WORKGROUP) if row.lone else (3, 2 * ps.WORKGROUP)), (row, n, fgrid)
    near_half = 0
    for mem, pat, copies, at in zip(laid, J.pats, J.copies, J.starts):
        _, kept, _ = ps.screened(mem)
        body = [c for c in copies if c.index >= 0]
        # every kept variant is in the text, where the layout says
        assert {c.index for c in body} == set(range(len(kept)))
        assert all(J.text[c.start:c.end] == kept[c.index].data for c in body)
        # every slot 0 .. k of the member -- A's last and B's first among them, either side of the piece_member
        # boundary -- is the only intact piece of some copy
        assert _sole_survivors(J.text, body, pat, mem.k, row.q) == set(range(mem.k + 1)), (row, mem)
        # ... and of copies whose match ends at each of the block offsets 62, 63, 0, 1
        for p in range(mem.k + 1):
            assert {(c.end - 1) % 64 for c in body if c.tag[0] == p} >= set(fa.END_OFFSETS), (row, mem, p)
        lane = sum(fa.straddles(c, 64 * 8) for c in body)
        wave = sum(fa.straddles(c, 64 * 64 * 8) for c in body)
        group = sum(fa.straddles(c, ps.WORKGROUP) for c in body)
        assert lane >= 20 and wave >= 1 and group >= 1, (row, mem, lane, wave, group)
        near_half += sum(0 <= c.end - half <= 64 and c.start < half for c in body)
        print(f"pair {ps.row_id(row)} member {mem_id(mem)} at {at}: copies {len(body)}, over lane / wave / workgroup borders "
              f"{lane} / {wave} / {group}")
    assert near_half >= 1, (row, half)
    # the oracle on the whole text: nearly every copy is a match of its own pattern, and the members' matches differ
    t0 = time.perf_counter()
    want = [oracle.search("dna", p, J.text, k, all_minima=True) for p, k in zip(J.pats, J.ks)]
    dt = time.perf_counter() - t0
    for mem, w, copies in zip(laid, want, J.copies):
        ends, found, j = sorted((x.text_start, x.text_end) for x in w), 0, 0
        for c in copies:  # (in text order)
            while j < len(ends) and ends[j][1] <= c.start:
                j += 1
            found += any(a < c.end and b > c.start for a, b in ends[j:j + 64])
        assert found * 100 >= 95 * len(copies), (row, mem, found, len(copies))
    spans = [{(x.text_start, x.text_end, x.cost) for x in w} for w in want]
    assert spans[0] != spans[1] and len(spans[0] ^ spans[1]) >= 100, (row, len(spans[0]), len(spans[1]))
    print(f"pair {ps.row_id(row)}: {n} bytes, oracle matches {[len(w) for w in want]}, {dt:.2f} s")


def test_mixed_text():
    """The cross-shape text: four layouts of four piece lengths, below 1 MiB, every variant of every member present."""
    J = ps.mixed_text(ps.MIXED)
    assert len(J.text) % 64 == 0 and len(J.text) < (1 << 20) and len(J.copies) == 4
    for mem, copies in zip(ps.MIXED, J.copies):
        _, kept, _ = ps.screened(mem)
        assert {c.index for c in copies if c.index >= 0} == set(range(len(kept)))
        assert sum(fa.straddles(c, ps.WORKGROUP) for c in copies) >= 1, mem
    twin = ps.mixed_text([ps.MIXED[0], ps.MIXED_TWIN, ps.MIXED[2], ps.MIXED[3]], ps.MIXED)
    assert twin.text == J.text and twin.pats[1] != J.pats[1] and len(twin.pats[1]) == 40
