"""CPU-only: the prefilter adversary (tests/helpers/filter_adversary.py) against the oracle -- it is not vacuous.  Every
variant of every shape really costs k (at most 2 % of a shape's variants may not, and leave), the piece it names is the
one that survives and the match end lies rem +- k from it, the q-gram variants keep exactly as many q-grams as they say
and reach the lemma's threshold, and the layout puts the copies on both sides of every block, lane, wave and workgroup
border that tests/test_gpu_filter_adversary.py relies on."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import filter_adversary as fa  # noqa: E402
import oracle  # noqa: E402

SHAPES = list(fa.SHAPES)
ids = lambda s: f"m{s[0]}k{s[1]}"


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle.build()


_screened = {}


def screened(pat, k, geo):
    """(kept, dropped) of the geometry's variants through the oracle (Dna profile), once per module."""
    if (pat, k, geo) not in _screened:
        _screened[(pat, k, geo)] = fa.screen(oracle.search, "dna", pat, k, fa.variants_for(pat, k, geo), random.Random(5))
    return _screened[(pat, k, geo)]


def _pieces_of(m, k, geo):
    return fa.multi_bounds(m, k) if geo[0] == "multi" else fa.piece_bounds(geo[1], k + 1)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_oracle_agreement(shape):
    """Alone in filler, every variant has an oracle match over it of cost exactly k and none cheaper; per shape at most
    2 % of the variants miss that (they leave the layout), and every (survivor, kind, layout) class keeps a variant."""
    m, k = shape
    pat = fa.shape_pattern(m, k)
    total = dropped_n = 0
    for geo in fa.shape_geometries(m, k):
        kept, dropped = screened(pat, k, geo)
        total += len(kept) + len(dropped)
        dropped_n += len(dropped)
        assert all(v.length == len(v.data) and len(v.tag) == 3 for v in kept)
        lost = {v.tag for v in dropped} - {v.tag for v in kept}
        assert not lost, (shape, geo, sorted(lost))
        kinds = {v.tag[1] for v in kept}
        assert kinds >= ({"sub", "ins", "del"} if geo[0] == "pair" else set(fa.KINDS)), (shape, geo, kinds)
        if geo[0] in ("pieces", "multi"):
            assert {v.tag[0] for v in kept} == set(range(k + 1)) and {v.tag[2] for v in kept} >= {"mid", "border"}
            # all k edits next to the survivor: both sides exist, for exactly the survivors whose run of k rows keeps
            # k + 1 + (k + 3) // 4 intact rows on either side (pinned here, so that the rule cannot thin them out unseen)
            need, bounds = k + 1 + (k + 3) // 4, _pieces_of(m, k, geo)
            behind = {p for p, (s, e) in enumerate(bounds) if e >= need and m - (e + k) >= need}
            front = {p for p, (s, e) in enumerate(bounds) if s - k >= need and m - s >= need}
            assert behind and front, (shape, geo, behind, front)
            for kind in ("ins", "del"):
                assert {v.tag[0] for v in kept if v.tag[1:] == (kind, "behind")} == behind, (shape, geo, kind, behind)
                assert {v.tag[0] for v in kept if v.tag[1:] == (kind, "front")} == front, (shape, geo, kind, front)
    print(f"shape {shape}: variants {total}, dropped {dropped_n}")
    assert dropped_n * 50 <= total, (shape, dropped_n, total)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_survivor_property(shape):
    """Pigeonhole variants: with 'mid' and 'border' exactly one piece keeps its rows, the one the tag names, and bytes.find
    finds it (and, but for chance occurrences of a short piece, no other); with 'behind' / 'front' the survivor keeps its
    rows and the piece next to it on the edited side does not.  All insertions / deletions on one side: the copy ends
    rem + k / rem - k columns behind the survivor, or begins k columns later / earlier in front of it."""
    m, k = shape
    pat = fa.shape_pattern(m, k)
    for geo in fa.shape_geometries(m, k):
        if geo[0] not in ("pieces", "multi"):
            continue
        bounds = _pieces_of(m, k, geo)
        variants = fa.variants_for(pat, k, geo)
        alone = spread = extremes = 0
        # (pieces whose rows the pattern itself repeats elsewhere: found wherever that repeat is intact)
        twice = {u for u, (s, e) in enumerate(bounds) if pat.find(pat[s:e], pat.find(pat[s:e]) + 1) >= 0}
        for v in variants:
            p, kind, layout = v.tag
            s_p, e_p = bounds[p]
            placed = [u for u, (s, e) in enumerate(bounds)
                      if v.row_at[s] >= 0 and [v.row_at[j] - v.row_at[s] for j in range(s, e)] == list(range(e - s))]
            found = [u for u, (s, e) in enumerate(bounds) if v.data.find(pat[s:e]) >= 0]
            assert p in placed and set(placed) <= set(found), (shape, geo, v.tag)
            assert v.data[v.row_at[s_p]:v.row_at[s_p] + e_p - s_p] == pat[s_p:e_p]
            one_side = layout == "behind" or (layout in ("mid", "border") and p == 0)
            other_side = layout == "front" or (layout in ("mid", "border") and p == k)
            if layout in ("mid", "border"):
                assert placed == [p], (shape, geo, v.tag, placed)
                spread += 1
                alone += [u for u in found if u == p or u not in twice] == [p]
            else:
                gone = p + 1 if layout == "behind" else p - 1
                assert gone not in placed, (shape, geo, v.tag, placed)
            if kind in ("ins", "del") and (one_side or other_side):
                shift = k if kind == "ins" else -k
                if one_side:     # the match end, rem + k or rem - k behind the piece's last column
                    assert v.length - (v.row_at[e_p - 1] + 1) == (m - e_p) + shift, (shape, geo, v.tag)
                else:            # the longest / shortest span in front of the piece
                    assert v.row_at[s_p] == s_p + shift, (shape, geo, v.tag)
                extremes += 1
        # a piece of q rows (4 * 3^(q-1) strings without equal neighbours) turns up by chance in a copy of L bytes about
        # k L / (4 * 3^(q-1)) times: allow twice that share
        q = min(e - s for s, e in bounds)
        chance = 2.0 * k * (m + k) / (4 * 3 ** (q - 1))
        assert alone >= spread * (1.0 - chance), (shape, geo, alone, spread, chance)
        assert extremes >= 4, (shape, geo, extremes)  # rem + k, rem - k, and both spans in front


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_qgram_counts(shape):
    """q-gram variants: the intact count the helper reports equals the count over the copy's rows, never falls below the
    lemma's threshold t = m + 1 - (k+1) Q, and equals it for some phase -- the counting filter's equality case."""
    m, k = shape
    pat = fa.shape_pattern(m, k)
    for geo in fa.geometries(m, k):
        if geo[0] != "qgram":
            continue
        Q = geo[1]
        t = fa.qgram_threshold(m, k, Q)
        variants = fa.qgram_variants(pat, k, Q)
        assert {(v.tag[0], v.tag[1]) for v in variants} == {(r, kind) for r in range(Q) for kind in fa.KINDS}
        for v in variants:
            brute = sum(1 for o in range(m - Q + 1)
                        if v.row_at[o] >= 0 and [v.row_at[o + j] - v.row_at[o] for j in range(Q)] == list(range(Q)))
            assert brute == v.intact, (shape, Q, v.tag, brute, v.intact)
            in_text = sum(1 for o in range(m - Q + 1) if v.data.find(pat[o:o + Q]) >= 0)
            assert in_text >= v.intact >= t, (shape, Q, v.tag, in_text, v.intact, t)
        assert min(v.intact for v in variants) == t, (shape, Q, t)
        kept, _ = screened(pat, k, geo)
        assert min(v.intact for v in kept) == t, (shape, Q, "the equality case left with the dropped variants")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_layout_borders_and_geometry(shape):
    """The layout at the GPU test's length, for every geometry and both lengths: a multiple of 64 (+ 1), every variant
    present, cut copies at both ends of the text; per even lane chunk bpl in 8 .. 32 at least 20 copies over a lane border
    (64 bpl), one over a wave border (64 * 64 bpl), for bpl = 8 one over the workgroup border at 128 KiB; per survivor
    copy ends at each of the block offsets 62, 63, 0, 1; short and long filler."""
    m, k = shape
    pat = fa.shape_pattern(m, k)
    for geo in fa.shape_geometries(m, k):
        kept, _ = screened(pat, k, geo)
        for extra in (0, 1):
            text, copies = fa.lay_out(kept, random.Random(100 * m + k), fa.MIN_BYTES, pat, k, extra=extra)
            n = len(text)
            assert n >= fa.MIN_BYTES and n % 64 == extra
            assert set(text) <= set(b"ACGT")
            head, tail, body = copies[0], copies[-1], copies[1:-1]
            assert head.start == 0 and text[:head.end] == pat[head.tag[1]:] and head.tag[1] <= k
            assert tail.end == n and text[tail.start:] == pat[:m - tail.tag[1]] and tail.tag[1] <= k
            assert {c.index for c in body} == set(range(len(kept)))
            for a, b in zip(copies, copies[1:]):
                assert a.end + b.gap == b.start and b.gap >= 0
            for c in body:
                assert text[c.start:c.end] == kept[c.index].data and c.tag == kept[c.index].tag
            lanes, waves = {}, {}
            for bpl in range(8, 33, 2):
                lanes[bpl] = sum(fa.straddles(c, 64 * bpl) for c in copies)
                waves[bpl] = sum(fa.straddles(c, 64 * 64 * bpl) for c in copies)
                assert lanes[bpl] >= 20 and waves[bpl] >= 1, (shape, geo, bpl, lanes[bpl], waves[bpl])
            workgroup = sum(c.start < 4 * 64 * 64 * 8 < c.end for c in copies)
            assert workgroup >= 1, (shape, geo)
            for p in {c.tag[0] for c in body}:
                offsets = {(c.end - 1) % 64 for c in body if c.tag[0] == p}
                assert offsets >= set(fa.END_OFFSETS), (shape, geo, p, sorted(offsets))
            short = sum(c.gap < fa.RUN_MERGE_GAP for c in body)
            long_ = sum(c.gap > m + k + 64 for c in body)
            assert short >= 20 and long_ >= 20, (shape, geo, short, long_)
            if extra == 0:
                print(f"shape {shape} {geo}: copies {len(copies)}, lane borders {min(lanes.values())}..{max(lanes.values())}, "
                      f"wave borders {min(waves.values())}..{max(waves.values())}, workgroup border {workgroup}, "
                      f"short / long filler {short} / {long_}")
    # half of the plants reverse-complemented: both strands present, the copies still where the layout says
    kept, _ = screened(pat, k, fa.geometries(m, k)[0])
    text, copies = fa.lay_out(kept, random.Random(100 * m + k), fa.MIN_BYTES, pat, k,
                              rc=lambda b: oracle.reverse_complement("dna", b))
    body = copies[1:-1]
    assert min(sum(c.rc for c in body), sum(not c.rc for c in body)) >= len(body) // 3
    for c in body:
        data = kept[c.index].data
        assert text[c.start:c.end] == (oracle.reverse_complement("dna", data) if c.rc else data)
    assert {c.start % 64 for c in body if c.rc} >= {1, 0, 63, 62}
