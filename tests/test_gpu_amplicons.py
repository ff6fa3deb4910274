"""Searcher.hamming_amplicons on the device against tests/helpers/amplicon_ref.py (the join of the numpy restatement's Hamming
records): whole arrays compared field for field and in order, after the helper's answer is checked to be what the case means
to exercise."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import oracle  # noqa: E402
import amplicon_ref as aref  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 64 * 64  # bytes of text a wavefront of the scan owns
OTHER = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG"}  # a substitution that is a mismatch under Dna and Iupac


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


class DevText:
    """The parts of a device tensor the Python surface reads (data_ptr, numel, is_cuda, a 1-byte dtype), over a DeviceBuffer."""

    class _Byte:
        itemsize = 1

    dtype = _Byte()
    is_cuda = True

    def __init__(self, ptr: int, n: int):
        self._p, self._n = ptr, n

    def data_ptr(self):
        return self._p

    def numel(self):
        return self._n

    def is_contiguous(self):
        return True


def dna(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(letters) for _ in range(n))


def mutate(rng, window: bytes, subs: int) -> bytes:
    w = bytearray(window)
    for j in rng.sample(range(len(w)), subs):
        w[j] = rng.choice(OTHER[w[j]])
    return bytes(w)


def rc_of(profile, seq):
    return oracle.reverse_complement(profile, seq)


def plant(text: bytearray, profile, start, end, left: bytes, right: bytes):
    """A product [start, end): `left` at its start, reverse_complement(right) at its end (the right site is written first)."""
    r = rc_of(profile, right)
    text[end - len(r):end] = r
    text[start:start + len(left)] = left


def spans(a):
    return [(int(x["pair_idx"]), int(x["strand"]), int(x["start"]), int(x["end"])) for x in a]


def check(s, profile, pairs, text, k, lo, hi, rc, frac=None, where=None, want=None):
    if want is None:
        want = aref.expected(profile, pairs, text, k, lo, hi, rc, max_n_frac=frac)
    got = s.hamming_amplicons(pairs, text, k, lo, hi)
    assert got.dtype == aref.DTYPE, where
    assert aref.same(got, want), (where, len(got), len(want), spans(got)[:8], spans(want)[:8])
    return want


# ---------------------------------------------------------------- 1. borders
BORDER_STARTS = (0, 63, 64, 4095, 4096, 4096 - 19, 8191)
# partner start = start + L - 18 on bit 0 / bit 63 of its block, for L = 100 and L = 300
PARTNER_BIT_STARTS = ((46, 100, 0), (45, 100, 63), (38 + 4096, 300, 0), (37 + 4096, 300, 63))


def border_case(sassy, start, length, present, seed, n=3 * TILE, sub_f=1, sub_r=0):
    rng = random.Random(seed)
    F, R = dna(rng, 20), dna(rng, 18)
    text = bytearray(dna(rng, n))
    plant(text, "dna", start, start + length, mutate(rng, F, sub_f), R)
    if sub_r:
        at = start + length - 18
        text[at:at + 18] = mutate(rng, bytes(text[at:at + 18]), sub_r)
    s = sassy.Searcher("dna", rc=True)
    want = aref.expected("dna", [(F, R)], bytes(text), 1, 100, 300, True)
    assert spans(want) == ([(0, 0, start, start + length)] if present else []), (start, length)
    if present:
        assert (int(want[0]["fwd_cost"]), int(want[0]["rev_cost"])) == (sub_f, sub_r)
    check(s, "dna", [(F, R)], bytes(text), 1, 100, 300, True, where=(start, length), want=want)


@pytest.mark.parametrize("start", BORDER_STARTS)
def test_borders(sassy, start):
    for length, present in ((99, False), (100, True), (300, True), (301, False)):
        border_case(sassy, start, length, present, seed=start * 7 + length, sub_r=length % 3 == 0)


def test_borders_partner_on_bit_0_and_63_and_the_texts_last_byte(sassy):
    for start, length, bit in PARTNER_BIT_STARTS:
        assert (start + length - 18) % 64 == bit
        border_case(sassy, start, length, True, seed=start + length)
    for n in (3 * TILE, 3 * TILE - 37):
        for length in (100, 300):
            border_case(sassy, n - length, length, True, seed=n + length, n=n)  # the product ends at the text's last byte


# ---------------------------------------------------------------- 2. mask edges
def test_mask_edges(sassy):
    """One left hit at 200, min_len 100, max_len 528, a = 20, b = 18: the partner window is [282, 710], both ends mid-mask (bit
    26 of block 4, bit 6 of block 11).  R = A x 18, so a run of r T holds r - 17 partner sites."""
    rng = random.Random(5)
    F, R = dna(rng, 20, b"ACG"), b"A" * 18
    s0, lo, hi = 200, 282, 710
    assert lo % 64 == 26 and hi % 64 == 6 and lo == s0 + 100 - 18 and hi == s0 + 528 - 18
    text = bytearray(dna(rng, 2 * TILE, b"ACG"))  # no T: the only partner sites are the planted ones
    text[s0:s0 + 20] = F
    text[lo - 1:lo + 1 + 18] = b"T" * 20   # sites lo - 1, lo, lo + 1
    text[hi - 1:hi + 1 + 18] = b"T" * 20   # sites hi - 1, hi, hi + 1
    middle = (5 * 64 + 10, 7 * 64 + 40, 9 * 64 + 1)  # one site in each of blocks 5, 7, 9; blocks 6, 8, 10 hold none
    for at in middle:
        text[at:at + 18] = b"T" * 18
    want = check(sassy.Searcher("dna", rc=True), "dna", [(F, R)], bytes(text), 0, 100, 528, True)
    assert [int(x) - 18 for x in want["end"]] == [lo, lo + 1, *middle, hi - 1, hi] and not want["strand"].any()
    assert set(want["start"].tolist()) == {s0}


# ---------------------------------------------------------------- 3. orientations and profiles
def test_orientations_rc_and_forward_only(sassy):
    rng = random.Random(9)
    F, R = dna(rng, 20), dna(rng, 18)
    text = bytearray(dna(rng, 3 * TILE))
    plant(text, "dna", 1000, 1250, mutate(rng, F, 1), R)           # '+': F ... rc(R)
    plant(text, "dna", TILE + 4000, 2 * TILE + 100, R, mutate(rng, F, 2))  # '-': R ... rc(F), across a tile border
    text = bytes(text)
    both = check(sassy.Searcher("dna", rc=True), "dna", [(F, R)], text, 2, 50, 400, True)
    assert spans(both) == [(0, 0, 1000, 1250), (0, 1, TILE + 4000, 2 * TILE + 100)]
    assert [(int(x["fwd_cost"]), int(x["rev_cost"])) for x in both] == [(1, 0), (2, 0)]
    fwd = check(sassy.Searcher("dna", rc=False), "dna", [(F, R)], text, 2, 50, 400, False)
    assert spans(fwd) == [(0, 0, 1000, 1250)]


def test_iupac_degenerate_primers_and_text(sassy):
    rng = random.Random(10)
    F, R = b"ACGRTTYACGNACGTTGCAA", b"GGRACTYYACGTNACGTA"
    text = bytearray(dna(rng, 2 * TILE + 333))
    plant(text, "iupac", 500, 800, b"ACGATTCACGTACGTTGCAA", b"GGAACTCTACGTGACGTA")   # concrete bases under R, Y, N
    plant(text, "iupac", TILE - 10, TILE + 250, b"ACGRTTYACGNACGTTGCAA", b"GGGACTTCACGTNACGTA")  # degenerate text letters
    plant(text, "iupac", 6000, 6200, b"GGAACTCCACGTAACGTA", b"ACGGTTTACGCACGTTGCAC")  # '-', one mismatch in F's site
    want = check(sassy.Searcher("iupac", rc=True), "iupac", [(F, R)], bytes(text), 1, 100, 400, True)
    assert spans(want) == [(0, 0, 500, 800), (0, 0, TILE - 10, TILE + 250), (0, 1, 6000, 6200)]
    assert int(want[2]["fwd_cost"]) == 1


def test_same_primer_twice_gives_both_strands_on_one_span(sassy):
    rng = random.Random(11)
    F = dna(rng, 22)
    text = bytearray(dna(rng, 2 * TILE))
    plant(text, "dna", 4000, 4200, F, F)
    want = check(sassy.Searcher("dna", rc=True), "dna", [(F, F)], bytes(text), 1, 100, 300, True)
    assert spans(want) == [(0, 0, 4000, 4200), (0, 1, 4000, 4200)]


def test_overlapping_sites_and_a_reverse_site_in_front(sassy):
    rng = random.Random(12)
    F = dna(rng, 20)
    R = rc_of("dna", F[2:])  # reverse_complement(R) = F[2:]: the right site lies inside the left one, L = max(a, b) = 20
    assert len(R) == 18
    G = dna(rng, 20)
    text = bytearray(dna(rng, 2 * TILE))
    text[300:320] = F
    text[3000:3020] = G
    H = rc_of("dna", bytes(text[2995:3013]))  # its site begins 5 bytes in front of G's and ends inside it: L = 13 < max(a, b)
    text = bytes(text)
    want = check(sassy.Searcher("dna", rc=True), "dna", [(F, R), (G, H)], text, 0, 1, 300, True)
    assert spans(want) == [(0, 0, 300, 320)]
    # both of (G, H)'s sites are there: with a partner behind G's site the pair has its product
    assert spans(aref.expected("dna", [(G, H)], text[:3020] + rc_of("dna", H) + text[3038:], 0, 1, 300, False)) == [(0, 0, 3000, 3038)]


# ---------------------------------------------------------------- 4. dense: many emit launches, overlapping ranges
def dense_text(letters):
    rng = random.Random(21)
    text = bytearray(dna(rng, 5 * TILE, letters))
    for border in range(TILE, 5 * TILE, TILE):
        text[border - 150:border + 150] = aref.HAND_TEXT
    text = bytes(text)
    want = aref.expected("dna", [aref.HAND_PAIR], text, 0, 4, 80, True)
    assert len(want) >= 4 * 2 * aref.HAND_COUNT == 4 * 5402
    return text, want


@pytest.fixture(scope="module")
def dense():
    """Random ACGT around the stretches; and random AT, where nearly every block holds a site of every scanned pattern, so that
    two tiles' worth of items is what two tiles have and the ranges do advance one tile at a time."""
    return {letters: dense_text(letters) for letters in (b"ACGT", b"AT")}


@pytest.mark.parametrize("options", ({}, {"hamming_records": 1000}, {"hamming_items": 4 * 64 * 2},
                                     {"hamming_items": 4 * 64 * 2, "hamming_records": 1000}))
@pytest.mark.parametrize("letters", (b"ACGT", b"AT"))
def test_dense_stretches_across_every_tile_border(sassy, dense, letters, options):
    text, want = dense[letters]
    s = sassy.Searcher("dna", rc=True)
    for name, value in options.items():
        s.set_option(name, value)
    check(s, "dna", [aref.HAND_PAIR], text, 0, 4, 80, True, where=(letters, options), want=want)
    launches = s.stats()["scan_launches"]
    if "hamming_items" not in options:
        assert launches == 1, launches
    elif letters == b"AT":
        assert launches >= 4, launches  # two tiles per range, advancing one tile at a time: four ranges or more


# ---------------------------------------------------------------- 5. pairs and groups
def test_pairs_of_mixed_lengths_in_groups(sassy):
    rng = random.Random(31)
    lens = [(8, 40), (40, 8), (20, 20), (25, 18), (25, 30), (12, 33), (100, 21), (17, 17), (9, 9), (30, 31), (22, 8), (16, 24)]
    pairs = [(dna(rng, a), dna(rng, b)) for a, b in lens]
    pairs[4] = (pairs[2][0], pairs[4][1])  # two pairs share a forward primer
    text = bytearray(dna(rng, 2 * TILE + 900))
    for i, (F, R) in enumerate(pairs):
        at = 150 + 700 * i
        if i == 4:
            at = 150 + 700 * 2  # behind the shared forward site of pair 2: a second reverse site
            r = rc_of("dna", R)
            text[at + 400 - len(r):at + 400] = r
            continue
        if i % 2:
            plant(text, "dna", at, at + 250 + i, mutate(rng, R, 1) if len(R) > 9 else R, F)  # '-'
        else:
            plant(text, "dna", at, at + 250 + i, F, mutate(rng, R, 1) if len(R) > 9 else R)  # '+'
    text = bytes(text)
    s = sassy.Searcher("dna", rc=True)
    want = check(s, "dna", pairs, text, 1, 60, 450, True)
    assert sorted(set(want["pair_idx"].tolist())) == list(range(12)) and set(want["strand"].tolist()) == {0, 1}
    s.set_option("hamming_batch", 8)  # four scanned patterns per pair: two pairs per launch group
    check(s, "dna", pairs, text, 1, 60, 450, True, want=want)
    assert s.stats()["scan_launches"] == 6
    s.set_option("hamming_batch", 1)  # a group holds at least one pair
    check(s, "dna", pairs, text, 1, 60, 450, True, want=want)
    assert s.stats()["scan_launches"] == 12
    s.set_option("hamming_batch", 0)
    # a pair with a primer longer than the text has no records and is no error
    short = text[:1000]
    more = pairs + [(dna(rng, 1024), dna(rng, 20)), (dna(rng, 20), dna(rng, 1001))]
    want = check(s, "dna", more, short, 1, 60, 450, True)
    assert len(want) >= 1 and max(want["pair_idx"].tolist()) < 12
    fwd = check(sassy.Searcher("dna", rc=False), "dna", pairs, text, 1, 60, 450, False)
    assert len(fwd) >= 5 and not fwd["strand"].any()


# ---------------------------------------------------------------- 6. max_n_frac
def test_max_n_frac_per_primer_site(sassy):
    rng = random.Random(41)
    F, R = dna(rng, 20), dna(rng, 18)
    two, three = bytearray(F), bytearray(F)
    for j in (3, 11):
        two[j] = ord("N")
    for j in (3, 11, 17):
        three[j] = ord("N")
    text = bytearray(dna(rng, 2 * TILE))
    plant(text, "iupac", 1000, 1200, bytes(two), R)    # 2 / 20 <= 0.1: at the threshold, stays
    plant(text, "iupac", 5000, 5200, bytes(three), R)  # 3 / 20: its forward site is dropped
    text = bytes(text)
    s = sassy.Searcher("iupac", rc=True)
    assert spans(check(s, "iupac", [(F, R)], text, 0, 100, 300, True)) == [(0, 0, 1000, 1200), (0, 0, 5000, 5200)]
    s.with_max_n_frac(0.1)
    assert spans(check(s, "iupac", [(F, R)], text, 0, 100, 300, True, frac=0.1)) == [(0, 0, 1000, 1200)]
    s.with_max_n_frac(0.0)
    assert len(check(s, "iupac", [(F, R)], text, 0, 100, 300, True, frac=0.0)) == 0


# ---------------------------------------------------------------- 7. device-resident text
def test_device_text_gives_the_host_array(sassy):
    rng = random.Random(51)
    F, R = dna(rng, 20), dna(rng, 18)
    text = bytearray(dna(rng, 3 * TILE + 7))
    plant(text, "dna", 60, 260, F, R)
    plant(text, "dna", 2 * TILE - 30, 2 * TILE + 90, R, mutate(rng, F, 1))
    plant(text, "dna", len(text) - 150, len(text), F, mutate(rng, R, 1))
    text = bytes(text)
    s = sassy.Searcher("dna", rc=True)
    want = check(s, "dna", [(F, R)], text, 1, 100, 300, True)
    assert len(want) == 3
    buf = sassy.DeviceBuffer(len(text) + 64)
    buf.upload(text)
    dev = DevText(buf.ptr, len(text))
    assert aref.same(s.hamming_amplicons([(F, R)], dev, 1, 100, 300), want)
    s.text_unchanged()
    assert aref.same(s.hamming_amplicons([(F, R)], dev, 1, 100, 300), want)
    s.text_unchanged(False)
    buf.free()


# ---------------------------------------------------------------- 8. tie to the engine on the device
def test_equals_the_join_of_the_devices_own_hamming_records(sassy):
    rng = random.Random(61)
    text = dna(rng, 64 * 1024)
    pairs = []
    for i in range(6):
        s0 = 3000 + 9000 * i
        length = (50, 3000, 700, 51, 2999, 1234)[i]
        F = text[s0:s0 + 18 + i]
        R = rc_of("dna", text[s0 + length - 21:s0 + length])
        if i % 2:  # written as the '-' orientation: the product's left site is the pair's reverse primer
            F, R = rc_of("dna", text[s0 + length - 21:s0 + length]), text[s0:s0 + 18 + i]
        pairs.append((F, R))
    s = sassy.Searcher("dna", rc=True)
    want = []
    for i, (F, R) in enumerate(pairs):
        hits = s.search_hamming([F, R], text, 2, without_trace=True)
        want.extend(aref.join(hits, i, len(F), len(R), 50, 3000, True))
    want = np.array(want, dtype=aref.DTYPE)
    assert sorted(set(want["pair_idx"].tolist())) == list(range(6))  # at least one product per pair by construction
    got = s.hamming_amplicons(pairs, text, 2, 50, 3000)
    assert aref.same(got, want), (spans(got), spans(want))


# ---------------------------------------------------------------- 9. emptiness
def test_emptiness(sassy):
    rng = random.Random(71)
    F, R = dna(rng, 20), dna(rng, 18)
    text = bytearray(dna(rng, 2 * TILE, b"ACG"))
    text[100:120] = F  # a forward site, no reverse site anywhere
    text = bytes(text)
    s = sassy.Searcher("dna", rc=True)
    for lo, hi in ((50, 500), (2 * TILE + 1, 3 * TILE)):  # no site of one primer; min_len beyond the text
        want = aref.expected("dna", [(F, R)], text, 1, lo, hi, True)
        got = s.hamming_amplicons([(F, R)], text, 1, lo, hi)
        assert len(want) == 0 and len(got) == 0 and got.dtype == aref.DTYPE and got.dtype == sassy.amplicon_dtype()
    assert len(s.hamming_amplicons([(F, R)], b"", 1, 1, 10)) == 0


# ---------------------------------------------------------------- 10. refusals that need a device
def test_open_tickets_refuse_the_call(sassy):
    text = dna(random.Random(11), 5000)
    buf = sassy.DeviceBuffer(len(text) + 64)
    buf.upload(text)
    s = sassy.Searcher("dna", rc=False)
    ticket = s.search_shard_begin(text[100:120], buf.ptr, 0, len(text), 0, len(text), 1)
    pair = (text[100:120], rc_of("dna", text[300:320]))
    with pytest.raises(sassy.SassyHipError, match="in flight"):
        s.hamming_amplicons([pair], text, 0, 50, 500)
    assert len(s.search_finish(ticket).matches) >= 1
    assert spans(s.hamming_amplicons([pair], text, 0, 50, 500)) == [(0, 0, 100, 320)]
    buf.free()


# ---------------------------------------------------------------- 11. CLI
def test_cli_amplicon(sassy, tmp_path, capsys):
    from sassy_amd import cli
    rng = random.Random(81)
    primers = [("p1", dna(rng, 20), dna(rng, 18)), ("p2", dna(rng, 16), dna(rng, 24))]
    chr1, chr2 = bytearray(dna(rng, TILE + 500)), bytearray(dna(rng, 3000))
    plant(chr1, "iupac", 200, 420, primers[0][1], mutate(rng, primers[0][2], 1))
    plant(chr1, "iupac", TILE - 50, TILE + 150, primers[1][2], primers[1][1])  # '-'
    plant(chr2, "iupac", 1000, 1300, mutate(rng, primers[1][1], 1), primers[1][2])
    fa = tmp_path / "t.fa"
    fa.write_bytes(b">chr1\n" + bytes(chr1) + b"\n>chr2\n" + bytes(chr2) + b"\n")
    tsv = tmp_path / "primers.tsv"
    tsv.write_bytes(b"".join(n.encode() + b"\t" + f + b"\t" + r + b"\n" for n, f, r in primers))
    pairs = [(f, r) for _, f, r in primers]
    for flags, rc in (([], True), (["--no-rc"], False)):
        rows, n = [cli.AMPLICON_HEADER[:-1] + "\tproduct\n"], 0
        for name, seq in (("chr1", bytes(chr1)), ("chr2", bytes(chr2))):
            want = aref.expected("iupac", pairs, seq, 1, 100, 400, rc)
            n += len(want)
            for x in want:
                product = seq[int(x["start"]):int(x["end"])]
                if x["strand"]:
                    product = rc_of("iupac", product)
                rows.append(f"{primers[int(x['pair_idx'])][0]}\t{name}\t{'-' if x['strand'] else '+'}\t{int(x['start'])}\t{int(x['end'])}\t"
                            f"{int(x['end']) - int(x['start'])}\t{int(x['fwd_cost'])}\t{int(x['rev_cost'])}\t{product.decode()}\n")
        assert n == (3 if rc else 2)
        assert cli.main(["amplicon", str(tsv), str(fa), "-k", "1", "--min-len", "100", "--max-len", "400", "--seq"] + flags) == 0
        assert capsys.readouterr().out == "".join(rows)
