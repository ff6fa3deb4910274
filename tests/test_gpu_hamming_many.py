"""Searcher.search_hamming_many / hamming_best_pattern on the device against tests/helpers/hamming_many_ref.py (the single-text
numpy restatement per text): whole records compared for equality, order included; the CLI's batch rows against the
per-record calls."""
import functools
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import oracle  # noqa: E402
import hamming_ref as href  # noqa: E402
import hamming_many_ref as mref  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 64 * 64  # bytes of text a wavefront owns (hamming_step.h: kHamTileBlocks blocks of 64)
BORDER_MS = (1, 6, 23, 64, 65, 130)
BORDER_KS = (0, 1, 3)


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


def dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def mutate(rng, window, subs, letters=b"ACGT"):
    w = bytearray(window)
    for _ in range(subs):
        w[rng.randrange(len(w))] = rng.choice(letters)
    return bytes(w)


# ---------------------------------------------------------------- (1) borders
@functools.lru_cache(maxsize=None)
def border_case(m):
    """(pattern, texts): every length of the issue's list, the pattern planted at start 0 and at len - m of every text that
    holds it, empty texts first, in the middle and last."""
    rng = random.Random(100 + m)
    pattern = dna(rng, m)
    lengths = sorted({1, m - 1, m, m + 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097} - {0})
    texts = [b"", b""]
    for i, n in enumerate(lengths):
        t = bytearray(dna(rng, n))
        if n >= m:
            if n >= 3 * m + 2:
                t[m + 1:2 * m + 1] = mutate(rng, pattern, 1 + i % 3)  # (a worse copy in between)
            t[0:m] = pattern
            t[n - m:n] = pattern
        texts.append(bytes(t))
        if i == len(lengths) // 2:
            texts += [b"", b"", b""]
    texts += [b"", b""]
    return pattern, tuple(texts)


@functools.lru_cache(maxsize=None)
def border_expected(m, k):
    pattern, texts = border_case(m)
    return tuple(mref.expected_many("dna", pattern, texts, k, rc=True))


@pytest.mark.parametrize("m", BORDER_MS)
def test_borders(sassy, m):
    pattern, texts = border_case(m)
    assert texts[0] == b"" and texts[-1] == b"" and b"" in texts[3:-3] and {len(t) for t in texts} >= {0, 1, m, 64, 4095, 4096, 4097}
    s = sassy.Searcher("dna", rc=True)
    for k in BORDER_KS:
        want = border_expected(m, k)
        with_hits = {t for t, _ in want}
        assert with_hits == {i for i, t in enumerate(texts) if len(t) >= m}, (m, k)  # every non-trivial text contributes
        ends = {(t, x.text_start) for t, x in want}
        assert all((i, len(t) - m) in ends for i, t in enumerate(texts) if len(t) >= m)
        assert all((i, 0) in ends for i, t in enumerate(texts) if len(t) >= 2 * m)  # (below 2 m the second plant overwrites the first)
        got = s.search_hamming_many(pattern, list(texts), k)
        assert mref.key_matches(got) == mref.key_many(want), (m, k)
        assert all(x.pattern_start == 0 and x.pattern_end == m for x in got)
    st = s.stats()
    assert st["filtered"] == 7 and st["scan_launches"] >= 1


# ---------------------------------------------------------------- (2) decoys that bite
def decoy_case():
    pattern = b"ACGGTCATTGCAAGCT"  # m = 16
    half = len(pattern) // 2
    texts = []
    for j in (1, 2, 64):  # (a) a text of exactly 64 j bytes that ends in the first half, the next begins with the second
        texts.append((b"AC" * (32 * j))[:64 * j - half] + pattern[:half])  # (no run of a letter, no G / T: no other hit)
        texts.append(pattern[half:] + b"CA" * 11)
    pats = [pattern]
    for letter in b"ACGT":  # (b) 62 bytes ending in four of a letter: the pattern of six reaches two bytes into the padding
        other = bytes(c for c in b"ACGT" if (c >> 1) & 3 != (letter >> 1) & 3)
        texts.append((other * 20)[:58] + bytes([letter]) * 4)
        pats.append(bytes([letter]) * 6)
    return pats, texts


def test_decoys_that_bite(sassy):
    pats, texts = decoy_case()
    pattern, half = pats[0], len(pats[0]) // 2
    want = mref.expected_many("dna", pats, texts, 0, rc=False)
    # (a) is live by construction: on the concatenation -- what the laid-out buffer holds, as these texts are whole blocks --
    # the straddling window is a hit, and the batch's definition has no hit there
    for i in (0, 2, 4):
        glued = texts[i] + texts[i + 1]
        at = len(texts[i]) - half
        assert len(texts[i]) % 64 == 0 and at in [x.text_start for x in href.expected("dna", pattern, glued, 0)]
        assert not [1 for t, x in want if t in (i, i + 1) and x.pattern_idx == 0]
    # (b) whatever code the padding byte has, one of the four patterns matches into it: with any of the four bytes behind
    # the text the window at 58 is a hit of the letter's pattern
    for j, letter in enumerate(b"ACGT"):
        t = texts[6 + j]
        assert len(t) == 62 and [x.text_start for x in href.expected("dna", pats[1 + j], t + bytes([letter]) * 2, 0)] == [58]
        assert not [1 for ti, x in want if ti == 6 + j]
    assert want == []
    s = sassy.Searcher("dna", rc=False)
    assert s.search_hamming_many(pats, texts, 0) == []
    # and with two mismatches allowed the same texts have hits, none of them across a text's end
    want2 = mref.expected_many("dna", pats, texts, 2, rc=True)
    assert {(6 + j, 1 + j, 56) for j in range(4)} <= {(t, x.pattern_idx, x.text_start) for t, x in want2}
    s = sassy.Searcher("dna", rc=True)
    assert mref.key_matches(s.search_hamming_many(pats, texts, 2)) == mref.key_many(want2)
    cost, pat, strand, start = s.hamming_best_pattern(pats, texts, 0)
    assert set(cost.tolist()) == {mref.NO_MATCH}


# ---------------------------------------------------------------- (3) more texts than lanes
@functools.lru_cache(maxsize=None)
def lanes_case():
    rng = random.Random(3)
    pattern = dna(rng, 8)
    texts = []
    for i in range(200):
        n = 1 + (i * 37) % 64  # every length 1 .. 64 (37 is coprime to 64), one block each
        t = bytearray(dna(rng, n))
        if n >= 8:
            at = rng.choice([0, n - 8, rng.randrange(0, n - 7)])
            t[at:at + 8] = mutate(rng, pattern, i % 3)
        texts.append(bytes(t))
    return pattern, tuple(texts)


def test_more_texts_than_lanes(sassy):
    pattern, texts = lanes_case()
    assert {len(t) for t in texts} == set(range(1, 65)) and len(texts) * 64 > 3 * TILE
    want = mref.expected_many("dna", pattern, texts, 1, rc=True)
    assert len({t for t, _ in want}) > 100
    got = sassy.Searcher("dna", rc=True).search_hamming_many(pattern, list(texts), 1)
    assert mref.key_matches(got) == mref.key_many(want)
    assert all(0 <= x.text_start and x.text_end <= len(texts[x.text_idx]) for x in got)


# ---------------------------------------------------------------- (4) the halo in the next text
@functools.lru_cache(maxsize=None)
def halo_case(m):
    rng = random.Random(40 + m)
    pattern = dna(rng, m)
    h = m // 2
    texts = []
    for n in (4095, 4096, 4097):
        texts.append(dna(rng, n - m) + pattern)                      # the plant ends exactly at the text's end
        texts.append(pattern[h:] + dna(rng, 50))                     # ... and the next text starts with the pattern's tail
        texts.append(dna(rng, n - h) + pattern[:h])                  # a text that ends in the pattern's head
        texts.append(pattern[h:] + dna(rng, 70))
    return pattern, tuple(texts)


@pytest.mark.parametrize("m", [130, 1024])
def test_halo_into_the_next_text(sassy, m):
    pattern, texts = halo_case(m)
    h = m // 2
    for k in (0, 2):
        want = mref.expected_many("dna", pattern, texts, k, rc=True)
        assert [(t, x.text_start) for t, x in want if x.strand == "+" and x.cost == 0] == [(0, 4095 - m), (4, 4096 - m), (8, 4097 - m)]
        # the whole-block text glued to its follower holds a hit across the seam that the batch must not report
        assert 4096 - h in [x.text_start for x in href.expected("dna", pattern, texts[6] + texts[7], 0)]
        assert not [1 for t, x in want if t in (6, 7) and x.cost == 0]
        got = sassy.Searcher("dna", rc=True).search_hamming_many(pattern, list(texts), k)
        assert mref.key_matches(got) == mref.key_many(want), (m, k)


# ---------------------------------------------------------------- (5) profiles
@functools.lru_cache(maxsize=None)
def iupac_case():
    rng = random.Random(5)
    pattern = b"ACGTTGCAACGGATCAGTCA"  # m = 20: 0.1 allows two N
    pats = (pattern, b"ACGRYTNACG")
    texts = []
    for run in (1, 2, 3, 5, 20, 64):
        texts.append(dna(rng, 40) + pattern[:10] + b"N" * run)         # a run of N ends the text ...
        texts.append(b"N" * run + pattern[10:] + dna(rng, 30))         # ... and the next begins with N
        texts.append(dna(rng, 64 - 12) + pattern[:8] + b"NN" + pattern[10:] + dna(rng, 7))
    texts.append(b"")
    texts.append(b"n" * 130)
    return pats, tuple(texts)


@pytest.mark.parametrize("frac", [0.0, 0.1])
def test_iupac_with_an_n_threshold(sassy, frac):
    pats, texts = iupac_case()
    for rc in (False, True):
        s = sassy.Searcher("iupac", rc=rc).with_max_n_frac(frac)
        for k in (1, 3):
            want = mref.expected_many("iupac", pats, texts, k, rc=rc, max_n_frac=frac)
            free = mref.expected_many("iupac", pats, texts, k, rc=rc)
            assert len(free) > len(want) and (want or frac == 0.0)
            assert mref.key_matches(s.search_hamming_many(pats, list(texts), k)) == mref.key_many(want), (frac, rc, k)


@functools.lru_cache(maxsize=None)
def ascii_case(wide):
    rng = random.Random(6 + wide)
    letters = b"abcdeABCDE[{_ "
    if wide:  # one pattern of more than 16 distinct bytes: the 64-slot kernels
        pats = (bytes(range(70, 100)), b"Hello_World")
    else:
        pats = (b"abcAB_de", b"{dE[a")
    texts = []
    for n in (0, 3, 40, 63, 64, 65, 128, 200, 4096, 4100):
        t = bytearray(rng.choice(letters) for _ in range(n))
        for p in pats:
            if n >= len(p):
                for at in (0, n - len(p)):
                    t[at:at + len(p)] = mutate(rng, p.swapcase() if at else p, 1 if at else 0, letters)
        texts.append(bytes(t))
    return pats, tuple(texts)


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("profile", ["ascii", "ascii_ci"])
def test_ascii_profiles(sassy, profile, wide):
    pats, texts = ascii_case(wide)
    s = sassy.Searcher(profile, rc=False)
    for k in (0, 2):
        want = mref.expected_many(profile, pats, texts, k)
        assert want
        assert mref.key_matches(s.search_hamming_many(pats, list(texts), k)) == mref.key_many(want), (profile, wide, k)


def test_without_trace_and_text_batch(sassy):
    pattern, texts = border_case(23)
    s = sassy.Searcher("dna", rc=True)
    want = mref.expected_many("dna", pattern, texts, 3, rc=True, without_trace=True)
    bare = s.search_hamming_many(pattern, list(texts), 3, without_trace=True)
    assert mref.key_matches(bare) == mref.key_many(want) and all(x.cigar == "" for x in bare)
    # a TextBatch (one buffer + offsets, what the FASTX reader holds) and the Result's array
    r = s.search_hamming_many([pattern], sassy.TextBatch.from_list(list(texts)), 3, as_result=True)
    assert mref.key_matches(r.matches) == mref.key_many(border_expected(23, 3))
    assert r.array["text_idx"].tolist() == [t for t, _ in want]


# ---------------------------------------------------------------- (6) seams
@pytest.mark.parametrize("m", BORDER_MS)
def test_seams_of_batches_ranges_and_pattern_groups(sassy, m):
    pattern, texts = border_case(m)
    pats = [pattern, pattern[: max(1, m // 2)] if m > 1 else b"G"]
    plain = sassy.Searcher("dna", rc=True)
    base = mref.key_matches(plain.search_hamming_many(pats, list(texts), 1))
    one = plain.stats()["scan_launches"]
    assert base == mref.key_many(mref.expected_many("dna", pats, texts, 1, rc=True))
    s = sassy.Searcher("dna", rc=True)
    s.set_option("hamming_many_batch", 8192).set_option("hamming_items", 64).set_option("hamming_batch", 1)
    assert mref.key_matches(s.search_hamming_many(pats, list(texts), 1)) == base, m
    s2 = sassy.Searcher("dna", rc=True)
    s2.set_option("hamming_many_batch", 8192)
    assert mref.key_matches(s2.search_hamming_many(pats, list(texts), 1)) == base, m
    assert s2.stats()["scan_launches"] >= 3 * one  # three texts of about 4 KiB: at least three batches
    best = [tuple(int(v) for v in row) for row in zip(*s.hamming_best_pattern(pats, list(texts), 1))]
    assert best == mref.expected_best("dna", pats, texts, 1, rc=True)


# ---------------------------------------------------------------- (7) the old path against the new
def test_single_text_calls_give_the_same_records(sassy):
    pattern, texts = border_case(23)
    texts = list(texts)
    assert len(texts) == 20
    s = sassy.Searcher("dna", rc=True)
    for k in (0, 3):
        many = s.search_hamming_many(pattern, texts, k)
        for t, text in enumerate(texts):
            single = s.search_hamming(pattern, text, k)
            mine = [x for x in many if x.text_idx == t]
            assert [href.key(x) for x in mine] == [href.key(x) for x in single], (k, t)
            assert all(x.text_idx == 0 for x in single)


# ---------------------------------------------------------------- (8) best pattern
def best_rows(s, pats, texts, k):
    return [tuple(int(v) for v in row) for row in zip(*s.hamming_best_pattern(pats, list(texts), k))]


def check_best(sassy, profile, pats, texts, k, rc, frac=None):
    s = sassy.Searcher(profile, rc=rc).with_max_n_frac(frac)
    got = best_rows(s, pats, texts, k)
    assert got == mref.expected_best(profile, pats, texts, k, rc=rc, max_n_frac=frac), (profile, k, rc, frac)
    own = s.search_hamming_many(pats, list(texts), k, without_trace=True)  # ... and the device's own records, reduced
    assert got == mref.reduce_best(len(texts), [(x.text_idx, x) for x in own])
    return got


def test_best_pattern_on_the_inputs_above(sassy):
    for m in BORDER_MS:
        pattern, texts = border_case(m)
        for k in BORDER_KS:
            got = check_best(sassy, "dna", [pattern], texts, k, True)
            assert [g[0] != mref.NO_MATCH for g in got] == [len(t) >= m for t in texts]
    pats, texts = decoy_case()
    check_best(sassy, "dna", pats, texts, 2, True)
    pattern, texts = lanes_case()
    check_best(sassy, "dna", [pattern], texts, 1, True)
    for m in (130, 1024):
        pattern, texts = halo_case(m)
        check_best(sassy, "dna", [pattern], texts, 2, True)
    pats, texts = iupac_case()
    for frac in (0.0, 0.1):
        check_best(sassy, "iupac", pats, texts, 3, True, frac)
    for profile in ("ascii", "ascii_ci"):
        for wide in (0, 1):
            pats, texts = ascii_case(wide)
            check_best(sassy, profile, pats, texts, 2, False)


def test_best_pattern_ties(sassy):
    rng = random.Random(8)
    bc = b"ACCGTTAGCATG"
    # the same barcode twice in a read: the leftmost; with a mismatch in the left one the right one (lower cost)
    twice = b"TT" + bc + b"GGGG" + bc + b"T"
    left_worse = b"TT" + bc[:5] + b"G" + bc[6:] + b"GGGG" + bc + b"T"
    # two patterns at equal cost: the lower index; the palindrome ACGT: Fwd
    two = b"AAAA" + b"GGGGCCCCAA" + b"TTTT" + b"GGGGCCCCAT" + b"A"
    s = sassy.Searcher("dna", rc=True)
    assert best_rows(s, [bc], [twice, left_worse], 1) == [(0, 0, 0, 2), (0, 0, 0, 18)]
    assert best_rows(s, [b"GGGGCCCCAT", b"GGGGCCCCAA"], [two], 1) == [(0, 0, 0, 18)]
    assert best_rows(s, [b"GGGGCCCCAG", b"GGGGCCCCAC"], [two], 1) == [(1, 0, 0, 4)]
    assert best_rows(s, [b"ACGT"], [b"TTTTACGTTTTT"], 0) == [(0, 0, 0, 4)]
    # a hit of the other strand only, behind a worse forward hit
    rcbc = oracle.reverse_complement("dna", bc)
    assert best_rows(s, [bc], [b"GG" + left_worse[2:14] + b"CC" + rcbc], 1) == [(0, 0, 1, 16)]
    texts = [twice, left_worse, two, dna(rng, 150), b"", b"ACG"]
    pats = [bc, b"GGGGCCCCAT", b"GGGGCCCCAA", b"ACGT"]
    got = best_rows(s, pats, texts, 1)
    assert got == mref.expected_best("dna", pats, texts, 1, rc=True)
    assert got[4] == got[5] == (mref.NO_MATCH, mref.NO_PATTERN, 0, mref.NO_START)


@pytest.mark.parametrize("k", [1, 3, 4, 15, 16, 200])
def test_best_pattern_at_every_plane_count(sassy, k):
    """k <= 254 reaches 2, 4 and 8 counter planes; every cost 0 .. k + 2 is planted once, in texts that also hold worse hits."""
    rng = random.Random(80 + k)
    m = 256 if k == 200 else 40
    pattern = dna(rng, m)
    other = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG"}
    costs = sorted(set(range(0, min(k, 20) + 3)) | {k - 1, k, k + 1})
    texts = []
    for c in costs:
        def window(cost):
            w = bytearray(pattern)
            for j in rng.sample(range(m), min(m, cost)):
                w[j] = rng.choice(other[w[j]])
            return bytes(w)
        texts.append(dna(rng, 30) + window(min(m, c + 1)) + dna(rng, 7) + window(c) + dna(rng, 61) + window(min(m, c + 2)))
    texts.append(dna(rng, 500))  # a read without a hit
    s = sassy.Searcher("dna", rc=True)
    got = best_rows(s, [pattern], texts, k)
    assert got == mref.expected_best("dna", [pattern], texts, k, rc=True)
    if k < 200:
        assert [g[0] for g in got[:-1]] == [c if c <= k else mref.NO_MATCH for c in costs] and got[-1][0] == mref.NO_MATCH
    else:  # (k = 200 of 256 rows: random windows are hits too, at about 190 mismatches -- the planted ones below that win)
        assert [g[0] for g in got[:23]] == costs[:23] and all(150 < g[0] <= k for g in got[23:])


# ---------------------------------------------------------------- (9) CLI
def test_cli_rows_are_the_per_record_rows(sassy, tmp_path, capsys):
    from sassy_amd import cli
    rng = random.Random(9)
    barcodes = [("bc%d" % i, dna(rng, 16 + i)) for i in range(5)]
    records = []
    for i in range(30):
        seq = bytearray(dna(rng, 40 + 7 * i))
        name, bc = barcodes[i % 5]
        if i % 6 != 5:
            w = mutate(rng, bc if i % 2 else oracle.reverse_complement("dna", bc), i % 3)
            at = rng.randrange(0, len(seq) - len(w) + 1)
            seq[at:at + len(w)] = w
        records.append(("read%d" % i, bytes(seq)))
    fq = tmp_path / "reads.fq"
    fq.write_text("".join(f"@{n}\n{s.decode()}\n+\n{'I' * len(s)}\n" for n, s in records))
    fa = tmp_path / "barcodes.fa"
    fa.write_text("".join(f">{n}\n{p.decode()}\n" for n, p in barcodes))
    s = sassy.Searcher("dna", rc=True).with_max_n_frac(0.2)
    pats = [p for _, p in barcodes]
    # the parent's output: one search_hamming call per record
    rows = ["pat_id\ttext_id\tcost\tstrand\tstart\tend\tmatch_region\tcigar\n"]
    for name, seq in records:
        rows += cli.hamming_rows(s, barcodes, name, seq, s.search_hamming(pats, seq, 2))
    assert len(rows) > 25
    assert cli.main(["search", "--hamming", "-a", "dna", "-f", str(fa), "-k", "2", str(fq)]) == 0
    assert capsys.readouterr().out == "".join(rows)
    assert cli.main(["demux", "-a", "dna", "-f", str(fa), "-k", "2", str(fq)]) == 0
    best = s.hamming_best_pattern(pats, [seq for _, seq in records], 2)
    want = cli.DEMUX_HEADER + "".join(cli.demux_rows(barcodes, [n for n, _ in records], best))
    assert capsys.readouterr().out == want
    assert want.count("\t*\t-1\t") >= 4 and want.count("\t-\t") >= 5 and want.count("\t+\t") >= 5


# ---------------------------------------------------------------- refusals that need a device
def test_open_tickets_refuse_the_batch_calls(sassy):
    text = dna(random.Random(11), 5000)
    buf = sassy.DeviceBuffer(len(text) + 64)
    buf.upload(text)
    s = sassy.Searcher("dna", rc=False)
    ticket = s.search_shard_begin(text[100:120], buf.ptr, 0, len(text), 0, len(text), 1)
    for call in (lambda: s.search_hamming_many([b"ACGT"], [text], 0), lambda: s.hamming_best_pattern([b"ACGT"], [text], 0)):
        with pytest.raises(sassy.SassyHipError, match="in flight"):
            call()
    assert len(s.search_finish(ticket).matches) >= 1
    assert s.hamming_best_pattern([text[100:120]], [text, b""], 0)[3].tolist() == [100, mref.NO_START]
    buf.free()
