"""Searcher.hamming_counts / hamming_counts_many on the device against tests/helpers/hamming_counts_ref.py (a bincount of the
numpy restatement's hits): whole tables compared for equality."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import oracle  # noqa: E402
import hamming_ref as href  # noqa: E402
import hamming_counts_ref as cref  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 64 * 64  # bytes of text a wavefront owns (hamming_step.h: kHamTileBlocks blocks of 64)
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


def on_device(sassy, text: bytes):
    buf = sassy.DeviceBuffer(len(text) + 64)
    if text:
        buf.upload(text)
    return buf, DevText(buf.ptr, len(text))


def dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def mutate(rng, window: bytes, subs: int) -> bytes:
    """`window` with exactly `subs` mismatching positions (ACGT windows)."""
    w = bytearray(window)
    for j in rng.sample(range(len(w)), subs):
        w[j] = rng.choice(OTHER[w[j]])
    return bytes(w)


def check(s, profile, pats, text, k, rc=False, frac=None, where=None):
    want = cref.expected_counts(profile, pats, text, k, rc=rc, max_n_frac=frac)
    got = s.hamming_counts(pats, text, k)
    assert got.dtype == np.uint64 and got.shape == want.shape, where
    assert np.array_equal(got, want), (where, got.tolist(), want.tolist())
    return want


# ---------------------------------------------------------------- borders
BORDER_MS = (1, 2, 63, 64, 65, 130, 1024)
BORDER_K = 2


def border_lengths(m):
    return sorted({m - 1, m, m + 1, 63, 64, 65, 4095, 4096, 4097, 2 * TILE + m, 3 * TILE + 7})


def border_places(n, m):
    """Starts at the first and last valid start, on either side of a 64-byte seam and of every 4 KiB seam of the text, and with
    the window straddling a seam (its tail in the next block / in the tile's halo)."""
    places = [0, n - m, 63, 64, 65 - m, 128 - m // 2]
    for seam in range(TILE, n + TILE, TILE):
        places += [seam - 1, seam, seam - m, seam - m + 1, seam - m // 2, seam - 64 - m // 3]
    return sorted({p for p in places if 0 <= p <= n - m})


def border_texts(rng, pattern, n):
    """Texts that together hold a window at every border place, non-overlapping inside a text, plant i with i % (k + 2)
    substitutions: (text, [(start, substitutions)])."""
    m = len(pattern)
    left = border_places(n, m)
    out = []
    i = 0
    while left:
        text = bytearray(dna(rng, n))
        planted, skipped, free_from = [], [], -1
        for at in left:
            if at <= free_from:
                skipped.append(at)
                continue
            subs = min(i % (BORDER_K + 2), m)
            text[at:at + m] = mutate(rng, pattern, subs)
            planted.append((at, subs))
            free_from = at + m  # (a gap of one byte: a neighbour's bytes never complete a window)
            i += 1
        out.append((bytes(text), planted))
        left = skipped
    if not out:
        out.append((dna(rng, n), []))
    return out


@pytest.mark.parametrize("m", BORDER_MS)
def test_borders(sassy, m):
    rng = random.Random(100 + m)
    pattern = dna(rng, m)
    s = sassy.Searcher("dna", rc=False)
    seen = 0
    for n in border_lengths(m):
        for text, planted in border_texts(rng, pattern, n):
            h = href.mismatches("dna", pattern, text)
            for at, subs in planted:
                assert h[at] == subs, (m, n, at)
            want = check(s, "dna", [pattern], text, BORDER_K, where=(m, n))
            if n < m:
                assert not want.any()
            seen += len(planted)
    assert seen >= 20


# ---------------------------------------------------------------- every cost at every plane count
@pytest.mark.parametrize("k", [0, 1, 3, 4, 15, 16, 200, 254])
def test_every_cost_at_every_plane_count(sassy, k):
    """Windows of every cost 0 .. k, and of k + 1 and k + 2, which must not be counted (m = 300 holds them all): the shape
    of test_every_value_of_h_at_every_threshold."""
    rng = random.Random(600 + k)
    m = 300
    pattern = dna(rng, m)
    parts = [dna(rng, 70)]
    for v in list(range(k + 3)) * 2:
        parts.append(mutate(rng, pattern, v) + dna(rng, rng.randrange(1, 9)))
    text = b"".join(parts)
    h = href.mismatches("dna", pattern, text)
    assert set(range(k + 3)) <= set(h.tolist())
    s = sassy.Searcher("dna", rc=False)
    want = check(s, "dna", [pattern], text, k, where=k)
    assert (want[0, 0] >= 2).all() and int(want.sum()) == int((h <= k).sum()) < int((h <= k + 2).sum())
    st = s.stats()
    assert st["candidates"] == int(want.sum()) and st["filtered"] == 7 and st["scan_launches"] == 1 and st["scan_ms"] > 0


# ---------------------------------------------------------------- dense and contended
def test_k_at_least_m_counts_every_start(sassy):
    rng = random.Random(7)
    text = dna(rng, 3 * TILE + 7)
    s = sassy.Searcher("dna", rc=True)
    for pats, k in (([b"ACGTA"], 5), ([b"ACGTA", b"GG"], 7), ([b"ACGTA", b"GG"], 3)):
        want = check(s, "dna", pats, text, k, rc=True, where=k)
        for p, pat in enumerate(pats):
            if k >= len(pat):
                assert int(want[p, 0].sum()) == int(want[p, 1].sum()) == len(text) - len(pat) + 1
                assert not want[p, :, len(pat) + 1:].any()  # bins with c > m


@pytest.mark.parametrize("copies", [0, 1, 4, 64])
@pytest.mark.parametrize("k", [0, 3])
def test_homopolymer_every_wave_adds_into_one_bin(sassy, k, copies):
    """256 KiB of A against A...A: every start is a hit of cost 0, every wavefront adds into one bin -- with the default
    number of table copies and with each forced one."""
    n, m = 256 * 1024, 20
    text = b"A" * n
    pats = [b"A" * m, b"A" * (m - 1) + b"C"]
    s = sassy.Searcher("dna", rc=True)
    s.set_option("hamming_count_copies", copies)
    want = check(s, "dna", pats, text, k, rc=True, where=(k, copies))
    assert int(want[0, 0, 0]) == n - m + 1 and int(want[0].sum()) == n - m + 1
    assert int(want[1].sum()) == (n - m + 1 if k >= 1 else 0) and (k == 0 or int(want[1, 0, 1]) == n - m + 1)
    assert s.stats()["candidates"] == int(want.sum())


# ---------------------------------------------------------------- strands
@pytest.mark.parametrize("profile", ["dna", "iupac"])
def test_strands(sassy, profile):
    rng = random.Random(31)
    plain, palindrome = dna(rng, 21), b"GAATTCGAATTC"
    assert oracle.reverse_complement(profile, palindrome) == palindrome
    pats = [plain, palindrome] + ([b"ACGRYNACGT"] if profile == "iupac" else [])
    text = bytearray(dna(rng, 2 * TILE + 300))
    for i, at in enumerate(range(50, len(text) - 40, 397)):
        pat = pats[i % len(pats)]
        w = pat if (i // len(pats)) % 2 == 0 else oracle.reverse_complement(profile, pat)
        w = bytes(rng.choice(b"ACGT") if c not in b"ACGT" else c for c in w)
        text[at:at + len(w)] = mutate(rng, w, i % 4)
    text = bytes(text)
    want = check(sassy.Searcher(profile, rc=True), profile, pats, text, 2, rc=True, where=profile)
    assert want[0, 0].any() and want[0, 1].any() and not np.array_equal(want[0, 0], want[0, 1])
    assert np.array_equal(want[1, 0], want[1, 1]) and want[1, 0].sum() >= 3  # the palindrome: both rows equal, both counted
    fwd = check(sassy.Searcher(profile, rc=False), profile, pats, text, 2, rc=False, where=profile)
    assert np.array_equal(fwd[:, 0], want[:, 0]) and not fwd[:, 1].any()


# ---------------------------------------------------------------- patterns
def test_mixed_patterns_groups_duplicates_and_too_long(sassy):
    rng = random.Random(41)
    n = 2 * TILE + 99
    pats = [dna(rng, 5), dna(rng, 64), dna(rng, 130), dna(rng, 23)]
    pats += [pats[0], dna(rng, n + 1 if n + 1 <= 1024 else 1024), pats[2]]
    text = bytearray(dna(rng, 1000))  # shorter than the 1024-row pattern
    for i, at in enumerate(range(3, 800, 150)):
        w = pats[i % 4]
        text[at:at + len(w)] = mutate(rng, w, min(i % 4, len(w)))
    text = bytes(text)
    assert len(pats[5]) > len(text)
    s = sassy.Searcher("dna", rc=True)
    want = check(s, "dna", pats, text, 3, rc=True)
    assert np.array_equal(want[0], want[4]) and np.array_equal(want[2], want[6]) and want[0].any() and want[2].any()
    assert not want[5].any()
    for batch, launches in ((1, 12), (3, 4), (0, 1)):  # 6 patterns fit the text, 12 scanned: groups are seamed
        s.set_option("hamming_batch", batch)
        assert np.array_equal(s.hamming_counts(pats, text, 3), want), batch
        assert s.stats()["scan_launches"] == launches, batch


# ---------------------------------------------------------------- the N rule
@pytest.mark.parametrize("frac", [0.0, 0.1, 0.5, None])
@pytest.mark.parametrize("profile", ["iupac", "dna"])
def test_n_rule(sassy, profile, frac):
    """Runs of N inside, across and around planted windows: a counted hit is a hit search_hamming would keep."""
    rng = random.Random(51)
    m, k = 20, 3
    pattern = dna(rng, m)
    text = bytearray(dna(rng, 2 * TILE + 50))
    at = 30
    for i, (n_from, n_len) in enumerate([(3, 1), (5, 2), (0, 3), (-4, 6), (m - 2, 9), (8, 10), (-30, 25), (m + 2, 12), (2, 40), (9, 0)] * 4):
        text[at:at + m] = mutate(rng, pattern, i % 3)
        text[at + n_from:at + n_from + n_len] = b"Nn"[i % 2:i % 2 + 1] * n_len
        at += 199
    text[TILE - 10:TILE + 30] = b"N" * 40  # a run across the tile's seam
    text = bytes(text)
    s = sassy.Searcher(profile, rc=True).with_max_n_frac(frac)
    want = check(s, profile, [pattern, pattern[:7]], text, k, rc=True, frac=frac, where=(profile, frac))
    loose = cref.expected_counts(profile, [pattern, pattern[:7]], text, k, rc=True)
    assert want.any() and (frac is not None or np.array_equal(want, loose))
    if profile == "iupac" and frac is not None:  # (an N of the text matches every Iupac letter: spans of N are hits until the rule drops them)
        assert int(want.sum()) < int(loose.sum())


# ---------------------------------------------------------------- Ascii
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("profile", ["ascii", "ascii_ci"])
def test_ascii_profiles(sassy, profile, wide):
    """Patterns with at most 16 distinct bytes, and with more (the NS 64 instantiation); ascii_ci in mixed case."""
    rng = random.Random(61 + wide)
    letters = b"abcdeABCDE[{_ " if not wide else bytes(range(48, 123))
    pats = [bytes(rng.choice(letters) for _ in range(m)) for m in ((9, 30) if not wide else (40, 70))]
    distinct = len({(c | 0x20 if profile == "ascii_ci" and chr(c).isalpha() else c) for p in pats for c in p})
    assert (distinct > 16) == bool(wide)
    text = bytearray(rng.choice(letters) for _ in range(TILE + 700))
    for i, at in enumerate(range(10, len(text) - 80, 331)):
        w = bytearray(pats[i % 2])
        if profile == "ascii_ci":
            w = bytearray(bytes(w).swapcase() if i % 3 else bytes(w).upper())
        for j in rng.sample(range(len(w)), i % 4):
            w[j] = 0x7E  # '~' is in no pattern
        text[at:at + len(w)] = w
    text = bytes(text)
    want = check(sassy.Searcher(profile, rc=False), profile, pats, text, 2, where=(profile, wide))
    assert want[0, 0].sum() >= 2 and want[1, 0].sum() >= 2 and not want[:, 1].any()


# ---------------------------------------------------------------- a text on the device
def test_device_text_gives_the_host_table(sassy):
    rng = random.Random(71)
    pats = [dna(rng, 23), dna(rng, 70)]
    text = bytearray(dna(rng, 3 * TILE + 7))
    for i, at in enumerate([0, 63, TILE - 1, TILE - 11, 2 * TILE - 35, 3 * TILE - 64, len(text) - 23, len(text) - 70]):
        w = pats[i % 2]
        if at + len(w) <= len(text):
            text[at:at + len(w)] = mutate(rng, w, i % 4)
    text = bytes(text)
    s = sassy.Searcher("dna", rc=True)
    want = check(s, "dna", pats, text, 3, rc=True)
    buf, dev = on_device(sassy, text)
    assert np.array_equal(s.hamming_counts(pats, dev, 3), want)
    s.text_unchanged()
    assert np.array_equal(s.hamming_counts(pats, dev, 3), want)
    assert np.array_equal(s.hamming_counts(pats[::-1], dev, 2), want[::-1, :, :3])
    s.text_unchanged(False)
    assert np.array_equal(s.hamming_counts(pats, dev, 3), want)
    buf.free()


# ---------------------------------------------------------------- a batch of texts
@pytest.mark.parametrize("m", [20, 130, 1024])
def test_batch(sassy, m):
    """Empty texts, texts shorter than the pattern, more texts than lanes; live decoys that straddle a text's end and reach
    into the padding (the pattern ends in A, the pad byte's code under Dna) or into the next text (the halo, m in {130,
    1024}); batches seamed.  The table is the sum of the single-text tables, and the helper's."""
    rng = random.Random(81 + m)
    pattern = dna(rng, m - 5) + b"AAAAA"
    short = dna(rng, 6) + b"AA"
    pats = [pattern, short]
    texts = [b"", dna(rng, 3), bytes(pattern), pattern[:-3], pattern[:-5] + b"C"]
    # the halo: a text that is whole blocks and ends in the pattern's head, the next one begins with its tail
    head = m // 2
    texts += [dna(rng, 4 * 64 - head) + pattern[:head], pattern[head:] + dna(rng, 50), b""]
    for i in range(70):
        t = bytearray(dna(rng, rng.choice([0, 5, m - 1, m, m + 1, 64, 2 * m + 17, TILE + 3])))
        if len(t) >= m:
            at = rng.choice([0, len(t) - m])
            t[at:at + m] = mutate(rng, pattern, i % 4)
        if len(t) >= len(short) + 2 and i % 5 == 0:
            t[len(t) - len(short) + 2:] = short[:-2]  # two bytes short of a hit: the padding would complete it
        texts.append(bytes(t))
    texts.append(mutate(rng, pattern, 1) + dna(rng, 2 * TILE))
    k = 2
    s = sassy.Searcher("dna", rc=True)
    want = cref.expected_counts("dna", pats, texts, k, rc=True)
    got = s.hamming_counts_many(pats, texts, k)
    assert got.dtype == np.uint64 and np.array_equal(got, want), (got.tolist(), want.tolist())
    assert s.stats()["candidates"] == int(want.sum()) and want[0, 0].all()
    assert np.array_equal(s.hamming_counts_many(pats, sassy.TextBatch.from_list(texts), k), want)
    s.set_option("hamming_many_batch", 8192).set_option("hamming_batch", 1)
    assert np.array_equal(s.hamming_counts_many(pats, texts, k), want)
    assert s.stats()["scan_launches"] > 8
    s.set_option("hamming_many_batch", 0).set_option("hamming_batch", 0)
    total = np.zeros_like(want)
    for t in texts:
        total += s.hamming_counts(pats, t, k)
    assert np.array_equal(total, want)


# ---------------------------------------------------------------- device against device
def test_large_device_text_against_the_record_path(sassy):
    """64 MiB generated on the device with planted hits: the table is the bincount of search_hamming's records (pattern,
    strand, cost) -- the tested record path as the reference at a size numpy should not be asked for."""
    n = 64 << 20
    rng = random.Random(91)
    pats = [b"ACGGTCATTGCATG", b"TTGACCGTAAGCTAGT"]
    k = 2
    buf = sassy.DeviceBuffer(n + 64)
    sassy.generate_dna(buf.ptr, n, 4343)
    for i, at in enumerate([0, TILE - 1, 4 * TILE - 5, 33 * (1 << 20) + 63, (1 << 25) - 7, n - 16 - 4096, n - 16]):
        w = pats[i % 2] if i % 3 else oracle.reverse_complement("dna", pats[i % 2])
        buf.upload(mutate(rng, w, i % 3), at)
    buf.upload(pats[0], n - len(pats[0]))
    s = sassy.Searcher("dna", rc=True)
    dev = DevText(buf.ptr, n)
    arr = s.search_hamming(pats, dev, k, without_trace=True, as_result=True).array
    strand = np.asarray(arr["strand"]).astype(np.int64)
    bins = (2 * arr["pattern_idx"].astype(np.int64) + strand) * (k + 1) + arr["cost"].astype(np.int64)
    want = np.bincount(bins, minlength=len(pats) * 2 * (k + 1)).astype(np.uint64).reshape(len(pats), 2, k + 1)
    got = s.hamming_counts(pats, dev, k)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert len(arr) >= 8 and want[:, 0].any() and want[:, 1].any() and s.stats()["candidates"] == len(arr)
    buf.free()


# ---------------------------------------------------------------- repeatability
def test_the_table_is_zeroed_between_calls(sassy):
    rng = random.Random(95)
    pattern = dna(rng, 12)
    dense, sparse = pattern * 300, dna(rng, 5000)
    s = sassy.Searcher("dna", rc=True)
    first = check(s, "dna", [pattern], dense, 4, rc=True)
    assert np.array_equal(s.hamming_counts([pattern], dense, 4), first) and first[0, 0, 0] == 300
    check(s, "dna", [pattern], sparse, 4, rc=True)
    check(s, "dna", [pattern, pattern], sparse, 1, rc=True)  # a larger table with fewer copies of it used before
    assert np.array_equal(s.hamming_counts([pattern], dense, 4), first)
    many = s.hamming_counts_many([pattern], [dense, sparse], 4)
    assert np.array_equal(s.hamming_counts_many([pattern], [dense, sparse], 4), many)
    assert np.array_equal(many, cref.expected_counts("dna", [pattern], [dense, sparse], 4, rc=True))


# ---------------------------------------------------------------- CLI
def test_cli_count(sassy, tmp_path, capsys):
    from sassy_amd import cli
    rng = random.Random(97)
    guides = [("g%d" % i, dna(rng, 18 + i)) for i in range(3)]
    records = []
    for i in range(6):
        seq = bytearray(dna(rng, [0, 10, 300, 700, 64, 5000][i]))
        for j, at in enumerate(range(20, len(seq) - 30, 97)):
            w = guides[j % 3][1] if j % 2 else oracle.reverse_complement("iupac", guides[j % 3][1])
            seq[at:at + len(w)] = mutate(rng, w, j % 4)
        if i == 3:
            seq[100:140] = b"N" * 40
        records.append(("chr%d" % i, bytes(seq)))
    fa = tmp_path / "genome.fa"
    fa.write_text("".join(f">{n}\n" + "".join(s[o:o + 60].decode() + "\n" for o in range(0, len(s), 60)) for n, s in records))
    pf = tmp_path / "guides.fa"
    pf.write_text("".join(f">{n}\n{p.decode()}\n" for n, p in guides))
    pats = [p for _, p in guides]
    k = 3
    for rc in (True, False):
        flags = ["--rc"] if rc else []
        want = cref.expected_counts("iupac", pats, [s for _, s in records], k, rc=rc)
        assert cli.main(["count", str(pf), str(fa), "-k", str(k)] + flags) == 0
        assert capsys.readouterr().out == cli.count_header(k) + "".join(cli.count_rows(guides, want, rc))
        assert want[:, 0].any() and (not rc or want[:, 1].any())
        rows = [cli.count_header(k, per_record=True)]
        for name, seq in records:
            rows += cli.count_rows(guides, cref.expected_counts("iupac", pats, seq, k, rc=rc), rc, text_id=name)
        assert cli.main(["count", str(pf), str(fa), "-k", str(k), "--per-record"] + flags) == 0
        assert capsys.readouterr().out == "".join(rows)
    # the N rule and another alphabet
    want = cref.expected_counts("dna", pats, [s for _, s in records], k, rc=True, max_n_frac=0.1)
    assert cli.main(["count", str(pf), str(fa), "-k", str(k), "--rc", "-a", "dna", "--max-n-frac", "0.1"]) == 0
    assert capsys.readouterr().out == cli.count_header(k) + "".join(cli.count_rows(guides, want, True))


# ---------------------------------------------------------------- refusals that need a device
def test_open_tickets_refuse_the_counting_calls(sassy):
    text = dna(random.Random(11), 5000)
    buf = sassy.DeviceBuffer(len(text) + 64)
    buf.upload(text)
    s = sassy.Searcher("dna", rc=False)
    ticket = s.search_shard_begin(text[100:120], buf.ptr, 0, len(text), 0, len(text), 1)
    for call in (lambda: s.hamming_counts([b"ACGT"], text, 0), lambda: s.hamming_counts_many([b"ACGT"], [text], 0)):
        with pytest.raises(sassy.SassyHipError, match="in flight"):
            call()
    assert len(s.search_finish(ticket).matches) >= 1
    assert s.hamming_counts([text[100:120]], text, 0).tolist() == [[[1], [0]]]
    buf.free()
