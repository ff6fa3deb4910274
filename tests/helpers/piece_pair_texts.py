"""Texts for the block-pair piece test of the grouped pass (pure Python and the oracle, no device).  The grouped launch tests
the pieces on two 64-byte blocks at once (csrc/piece_pair_step.h), so a block border is of one of two kinds: inside a pair or
between two pairs.  Per member pair one text of copies from the prefilter adversary (tests/helpers/filter_adversary.py) whose
ONLY intact piece is one named slot, placed by block:
  'even' / 'odd'       the intact piece's bytes straddle the border in front of an even / an odd block -- whichever way the
                       kernel pairs blocks, one of the two lies inside a pair and the other between pairs;
  'first' / 'second'   the intact piece lies wholly in one block, and the block behind (in front of) it holds the sole
                       intact piece of a copy of the OTHER member: both members hit in both blocks of one pair, once with
                       the even block first and once with the odd one;
and a text of exact copies of both members every 256 bytes, which makes every wave end segments in mid-stream.

Shared by tests/test_piece_pair_layout_cpu.py (the texts hold what they claim) and tests/test_gpu_piece_pair.py."""
import collections
import random

import filter_adversary as fa
import pass_shapes as ps

BLOCK = fa.BLOCK
KINDS = ("even", "odd", "first", "second")

# the bench's pair (two (32, 3) patterns: Q = 8, 4 + 4 slots), Q = 7 with 4 + 3 slots, Q = 12 with rows behind the last piece
ROWS = [r for r in ps.PAIRS if (r.a, r.b) in (((32, 3, 0), (32, 3, 1)), ((29, 3, 0), (21, 2, 0)), ((64, 3, 0), (48, 3, 0)))]
assert [r.q for r in ROWS] == [7, 8, 12] and not any(r.lone for r in ROWS)
# On a shard with a halo two searches share a launch only where they agree on the first block the chunk DP owns
# (ScanJob::group_fits: dp_first_owned), and 64 and 48 rows do not: there Q = 12 comes as two patterns of 64 rows, 4 + 4 slots.
HALO_ROWS = ROWS[:2] + [ps.Row(12, ps.M(64, 3), ps.M(64, 3, 1), False)]

# member: 0 / 1; slot: the intact piece; kind: above; start, end: the copy's bytes; lo, hi: the intact piece's bytes
Plant = collections.namedtuple("Plant", "member slot kind start end lo hi data")
# generated / dropped: per (member, slot) the sole-survivor variants the adversary makes and those the oracle's screen drops
PairText = collections.namedtuple("PairText", "text odd odd_blocks pats ks plants generated dropped")


def sole_survivors(member):
    """{slot: kept variants whose only intact piece is that slot}, and the generated and dropped counts per slot"""
    _, kept, dropped = ps.screened(member)
    sole = lambda vs: [v for v in vs if v.tag[2] in ("mid", "border")]  # noqa: E731
    by_slot = {p: [v for v in sole(kept) if v.tag[0] == p] for p in range(ps.n_pieces(member))}
    gone = {p: sum(1 for v in sole(dropped) if v.tag[0] == p) for p in by_slot}
    return by_slot, {p: len(by_slot[p]) + gone[p] for p in by_slot}, gone


def piece_span(member, v, slot):
    """[lo, hi): where the variant holds the rows of piece `slot`, untouched and in a row"""
    q = ps.piece_len(member.m, member.k)
    at = v.row_at[slot * q:(slot + 1) * q]
    assert at[0] >= 0 and at == list(range(at[0], at[0] + q)), (v.tag, slot, at)
    return at[0], at[0] + q


_texts = {}


def pair_text(row, min_bytes=fa.MIN_BYTES):
    if row in _texts:
        return _texts[row]
    members = (row.a, row.b)
    q = row.q
    rng = random.Random(7000 + 100 * row.a.m + row.b.m)
    info = [sole_survivors(mem) for mem in members]
    n_blocks = (min_bytes + BLOCK - 1) // BLOCK
    n_blocks += n_blocks & 1  # the whole text: an even count of blocks
    text = bytearray(fa.filler(rng, n_blocks * BLOCK))
    plants = []

    def put(mi, slot, kind, v, start):
        lo, hi = piece_span(members[mi], v, slot)
        assert start >= 0 and (not plants or start >= plants[-1].end + 2), (kind, start, plants[-1:])
        text[start:start + v.length] = v.data
        plants.append(Plant(mi, slot, kind, start, start + v.length, start + lo, start + hi, v.data))

    def up(x, parity):  # the first block number >= x of that parity
        return x + ((x ^ parity) & 1)

    cur, turn, second = 2, 0, [0, 0]
    last_room = n_blocks - 8  # (the last blocks: the two copies that end in the last block of the text and of odd_blocks)
    done = False
    while not done:
        for mi, mem in enumerate(members):
            for slot in range(ps.n_pieces(mem)):
                vs = info[mi][0][slot]
                assert vs, ("the screen left no sole-survivor copy of", mem, slot)
                for parity in (0, 1):
                    # the intact piece across the border in front of block B, every split of its q bytes in turn
                    v = vs[(2 * turn + parity) % len(vs)]
                    lo, _ = piece_span(mem, v, slot)
                    split = 1 + (turn + parity) % (q - 1)
                    B = up(cur + (split + lo + BLOCK - 1) // BLOCK, parity)
                    start = B * BLOCK - split - lo
                    if (start + v.length) // BLOCK + 3 >= last_room:
                        done = True
                        break
                    put(mi, slot, "odd" if parity else "even", v, start)
                    cur = (start + v.length) // BLOCK + 2 + rng.randrange(2)
                    # the intact piece at the front of block b, the other member's at the back of block b + 1
                    oi = 1 - mi
                    oslot = second[oi] % ps.n_pieces(members[oi])
                    second[oi] += 1
                    w = info[oi][0][oslot][turn % len(info[oi][0][oslot])]
                    v = vs[(2 * turn + parity + 1) % len(vs)]
                    lo, hi = piece_span(mem, v, slot)
                    wlo, _ = piece_span(members[oi], w, oslot)
                    b = up(cur + (lo + BLOCK - 1) // BLOCK, parity)
                    start, wstart = b * BLOCK - lo, (b + 2) * BLOCK - q - wlo
                    assert start + v.length + 2 <= wstart, (row, v.tag, w.tag)
                    if (wstart + w.length) // BLOCK + 3 >= last_room:
                        done = True
                        break
                    put(mi, slot, "first", v, start)
                    put(oi, oslot, "second", w, wstart)
                    cur = (wstart + w.length) // BLOCK + 2 + rng.randrange(2)
                if done:
                    break
            if done:
                break
        turn += 1
    # a copy that ends in the last block of the text less one block (an odd count of blocks), and one in the whole text's last
    for end in ((n_blocks - 1) * BLOCK - 40, n_blocks * BLOCK - 2):
        v = info[0][0][0][0]
        put(0, 0, "last", v, end - v.length)
    out = PairText(bytes(text), bytes(text[:-ps.ODD_CUT]), bytes(text[:-BLOCK]), [ps.pattern(x) for x in members], [x.k for x in members],
                   plants, [i[1] for i in info], [i[2] for i in info])
    _texts[row] = out
    return out


def dense_text(row, workgroups=3):
    """Exact copies of member 0 at every multiple of 256 bytes and of member 1 128 bytes behind, random bases between, over
    `workgroups` workgroups and a block: 128 windows per wave and member, twice the queue pressure a segment ends at."""
    rng = random.Random(11)
    pats = [ps.pattern(row.a), ps.pattern(row.b)]
    assert max(len(p) for p in pats) + row.a.k < 128
    n = workgroups * ps.WORKGROUP + BLOCK
    text = bytearray(fa.filler(rng, n))
    for at in range(0, n - 256, 256):
        text[at:at + len(pats[0])] = pats[0]
        text[at + 128:at + 128 + len(pats[1])] = pats[1]
    return bytes(text), pats, [row.a.k, row.b.k]
