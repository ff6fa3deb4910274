"""No GPU: the sizes of tests/helpers/scan_levels.py against the constants of the kernels they are meant to outgrow, read
out of the sources -- whoever retunes a constant gets a failing test here, not a GPU test that silently stops reaching the
level -- and the builders of that module: every plant sits where its comment says, every fast expectation equals the
helper's definition."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import fasta_ref  # noqa: E402
import hamming_pairs_ref as pref  # noqa: E402
import line_spans_ref  # noqa: E402
import scan_levels as lv  # noqa: E402

CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, pattern):
    found = re.findall(pattern, text)
    assert len(found) >= 1 and len(set(found)) == 1, (pattern, found)
    return int(found[0])


def constants(pairs=None, fasta=None, lines=None):
    pairs, fasta, lines = pairs or source("hamming_pairs.hip"), fasta or source("fasta_unwrap.hip"), lines or source("line_index.hip")
    c = {"scan_items": constant(pairs, r"kScanItems = (\d+)"),
         "scan_threads": constant(pairs, r"kScanBlock = (\d+) \* kScanItems"),
         "top_threads": constant(pairs, r"pairs_scan_top_kernel, dim3\(1\), dim3\((\d+)\)"),
         "tile_words": constant(pairs, r"kPairsTileWords = (\d+)"),
         "encode_threshold": 1 << constant(pairs, r"workers = n < \(1u << (\d+)\)"),
         "encode_workers": constant(pairs, r"std::min<size_t>\((\d+), std::max\(1u, std::thread::hardware_concurrency"),
         "tiles_per_super": constant(fasta, r"kTilesPerSuper = (\d+)"),
         "fasta_scan_threads": constant(fasta, r"fasta_scan_kernel, dim3\(1\), dim3\((\d+)\)"),
         "rec_per_thread": constant(fasta, r"kRecPerThread = (\d+)"),
         "rec_threads": constant(fasta, r"kRecBlock = (\d+) \* kRecPerThread"),
         "rec_top_threads": constant(fasta, r"fasta_rec_top_kernel, dim3\(1\), dim3\((\d+)\)"),
         "line_tiles_per_super": constant(lines, r"kLineTilesPerSuper = (\d+)"),
         "line_scan_threads": constant(lines, r"line_scan_kernel, dim3\(1\), dim3\((\d+)\)")}
    a, b = re.search(r"std::min<uint64_t>\(n_tiles, (\d+)u \* (\d+)u\)", fasta).groups()
    c["compact_grid"] = int(a) * int(b)
    # the loops that the launch widths above belong to
    assert re.search(r"b0 < n_blocks; b0 \+= %d\)" % c["top_threads"], pairs)
    assert len(re.findall(r"per = \(n_(?:super|blocks) \+ 1023\) / 1024", fasta)) == 2 and c["fasta_scan_threads"] == c["rec_top_threads"] == 1024
    assert re.search(r"per = \(n_super \+ 1023\) / 1024", lines) and c["line_scan_threads"] == 1024
    return c


def levels_reached(c):
    """every size of scan_levels.py lies beyond the threshold computed from the kernels' constants"""
    scan_block = c["scan_threads"] * c["scan_items"]
    assert scan_block == lv.SCAN_BLOCK
    blocks = [-(-n // scan_block) for n in lv.PAIRS_BLOCK_SIZES]
    assert blocks == [1, 1, 2, 3] and lv.PAIRS_BLOCK_SIZES[1] == scan_block            # one partial, one full, two, three
    assert all(-(-n // scan_block) >= 2 for n in lv.PAIRS_SELF_SIZES)
    n_blocks = -(-lv.PAIRS_TOP_N_A // scan_block)
    assert n_blocks > c["top_threads"] + 1 and lv.PAIRS_TOP_N_A % scan_block           # a second turn of two blocks, one partial
    assert lv.PAIRS_TOP_N_A >= c["encode_threshold"] and lv.ENCODE_N_B >= c["encode_threshold"]
    assert lv.ENCODE_WORKERS == c["encode_workers"]
    for _, P, m, W in lv.SEAM_CASES:
        assert W == (1 if m <= 32 else 2 if m <= 64 else 4) and lv.seam_T(P, W) == c["tile_words"] // (P * W)
    tile = 4096
    assert lv.TILE == tile and lv.SUPER == tile * c["tiles_per_super"] == tile * c["line_tiles_per_super"]
    n_super, n_tiles = -(-lv.FASTA_BIG // lv.SUPER), -(-lv.FASTA_BIG // tile)
    assert -(-n_super // c["fasta_scan_threads"]) >= 2 and n_super % 2                 # per >= 2, the last owning thread short
    assert n_tiles > 4 * c["compact_grid"] and c["compact_grid"] == 4096               # workgroup 0: tiles 0, 4096, ..., 16384
    rec_block = c["rec_threads"] * c["rec_per_thread"]
    assert rec_block == lv.REC_BLOCK
    assert -(-(-(-lv.FASTA_MANY_RECORDS // rec_block)) // c["rec_top_threads"]) >= 2 and lv.FASTA_MANY_RECORDS % rec_block
    n_super = -(-lv.LINES_BIG // lv.SUPER)
    assert -(-n_super // c["line_scan_threads"]) >= 2 and n_super % 2


def test_sizes_lie_beyond_the_kernels_thresholds():
    levels_reached(constants())


def test_a_retuned_constant_fails_this_test():
    """kScanItems, kTilesPerSuper or kRecPerThread doubled in a copy of the source: the sizes no longer reach the level"""
    for name, kwarg, old in (("hamming_pairs.hip", "pairs", "kScanItems = 8"), ("fasta_unwrap.hip", "fasta", "kTilesPerSuper = 16"),
                             ("fasta_unwrap.hip", "fasta", "kRecPerThread = 4"), ("line_index.hip", "lines", "kLineTilesPerSuper = 16")):
        text = source(name)
        assert text.count(old) == 1, old
        retuned = text.replace(old, old.split(" = ")[0] + " = " + str(2 * int(old.split(" = ")[1])))
        try:
            levels_reached(constants(**{kwarg: retuned}))
        except AssertionError:
            continue
        raise AssertionError(f"{old} doubled and every size still passes")


# ---------------------------------------------------------------- pairs
def rows_of_blocks(want, n_a):
    per_row = np.bincount(want["a_idx"], minlength=n_a)
    for b0 in range(0, n_a, lv.SCAN_BLOCK):
        block = per_row[b0:b0 + lv.SCAN_BLOCK]
        assert block.any() and (len(block) == 1 or not block.all()), b0
    return per_row


def test_pairs_block_cases_hold_empty_and_full_rows_in_every_block():
    for profile in ("dna", "iupac", "ascii"):
        for n_a in lv.PAIRS_BLOCK_SIZES:
            a, b, k = lv.pairs_block_case(profile, n_a, seed=n_a)
            assert a.shape == (n_a, 6) and 3 <= len(b) <= 8 and (a[lv.block_borders(n_a)] == b[0]).all()
            want = pref.expected_pairs(profile, a, b, k)
            per_row = rows_of_blocks(want, n_a)
            assert per_row[lv.block_borders(n_a)].all() and len(set(per_row.tolist())) >= 3, (profile, n_a)
            for g, w in zip(lv.nearest_fast(want, n_a), pref.expected_nearest(profile, a, b, k)):
                assert g.dtype == w.dtype and (g == w).all()
    assert lv.block_borders(4097) == [0, 2047, 2048, 4095, 4096]


def test_pairs_self_case_borders():
    a, k = lv.pairs_self_case("dna", True, 2049, seed=2050)
    assert (a[2047] == a[2048]).all() and a[2048].tobytes() == lv.revcomp("dna", a[2048]).tobytes()
    want, square = pref.expected_self("dna", a, k, True)
    assert rows_of_blocks(want, 2049)[[2047, 2048]].all()
    assert want.tobytes() == pref.expected_pairs("dna", a, None, k, True).tobytes()
    for g, w in zip(lv.nearest_fast(square, 2049), pref.expected_nearest("dna", a, None, k, True)):
        assert g.dtype == w.dtype and (g == w).all()


def test_pairs_top_case_rows():
    a, b, k = lv.pairs_top_case()
    n_a = lv.PAIRS_TOP_N_A
    borders = lv.block_borders(n_a)
    assert a.shape == (n_a, 4) and len(b) == 3 and {0, 2047, 2048, 1024 * 2048 - 1, 1024 * 2048, n_a - 1} <= set(borders)
    assert (a[borders] == b[0]).all()
    for rc in (False, True):
        want = pref.expected_pairs("dna", a, b, k, rc)
        per_row = rows_of_blocks(want, n_a)
        assert per_row[borders].all() and 200_000 < len(want) < 4_000_000 and (per_row == 0).mean() > 0.5, (rc, len(want))


def test_fast_nearest_equals_the_definition_on_the_border_cases():
    """scan_levels.nearest_fast against hamming_pairs_ref.nearest_of_pairs on border cases of tests/test_gpu_hamming_pairs.py"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_hamming_pairs as small
    for t in range(0, 48, 5):
        for self_mode in (False, True):
            profile, rc, m, k, chunks, a, b, want_pairs, want_nearest = small.border_case(t, self_mode)
            square = pref.expected_pairs(profile, a, b, k, rc, square=True)
            for g, w in zip(lv.nearest_fast(square, len(a)), want_nearest):
                assert g.dtype == w.dtype and (g == w).all(), (t, self_mode)
    for g, w in zip(lv.nearest_fast(np.zeros(0, dtype=pref.PAIR), 3), pref.nearest_of_pairs(np.zeros(0, dtype=pref.PAIR), 3)):
        assert g.dtype == w.dtype and (g == w).all()


def test_encode_case_plants():
    assert lv.encode_borders()[:4] == [0, 8749, 8750, 17499] and lv.encode_borders()[-1] == 70000 and len(lv.encode_borders()) == 16
    for profile in ("dna", "iupac"):
        a, b, k = lv.encode_case(profile, seed=7)
        assert a.shape == (3, 12) and len(b) == lv.ENCODE_N_B
        h = pref.distances(profile, a[:1], b[lv.encode_borders()], True)[0]
        for q in range(16):  # 0 .. k + 1 rows changed, every second one as the reverse complement
            assert h[q, q % 2] == q % (k + 2), (profile, q, h[q])


def test_seam_cases_hold_records_on_both_sides_of_every_seam():
    for profile, P, m, W in lv.SEAM_CASES:
        T, U = lv.seam_T(P, W), lv.seam_U(P, W)
        assert T in (64, 128, 256, 512, 1024) and U * P * W <= 32 and (U == 8 or 2 * U * P * W > 32)
        for rc in ((False, True) if profile != "ascii" else (False,)):
            S = 2 if rc else 1
            a, b, n_records = lv.seam_case(profile, P, m, W, rc, False)
            assert len(a) <= 300 and a.shape[1] == m and n_records == S * len(b) > 2 * T + 9
            present = lv.seam_records_present(pref.expected_pairs(profile, a, b, lv.SEAM_K, rc), S)
            assert set(lv.seam_records(T, n_records)) <= present, (profile, m, rc)
            a, _, n_records = lv.seam_case(profile, P, m, W, rc, True)
            assert n_records == S * len(a) > 2 * T + 9
            want = pref.expected_pairs(profile, a, None, lv.SEAM_K, rc)
            assert set(lv.seam_records(T, n_records)) <= lv.seam_records_present(want, S), (profile, m, rc)
            per_row = np.bincount(want["a_idx"], minlength=len(a))
            forced = lv.self_walk_chunks(len(a), S, T, U)
            seen = set()
            for chunks in (1, forced):
                kinds = lv.self_walk_kinds(len(a), S, T, chunks)
                seen |= set(kinds)
                for kind, waves in kinds.items():
                    assert any(per_row[i0:i0 + 64].any() for i0 in waves), (profile, m, rc, chunks, kind)
            assert {"at", "inside"} <= seen and ("behind" in seen or T > 192 * S), (profile, m, rc, sorted(seen))
            assert all(off % (64 * S) == 0 for _, off, _ in lv.self_walk_offsets(len(a), S, T, 1))
            assert any(0 < off < cnt and off % (U if U > S else 64 * S) for _, off, cnt in lv.self_walk_offsets(len(a), S, T, forced))


# ---------------------------------------------------------------- FASTA
def test_fasta_big_plants():
    S = lv.SUPER
    for variant in (0, 1):
        arr, at = lv.fasta_big(variant)
        raw = arr.tobytes()
        assert len(raw) == lv.FASTA_BIG and raw[:1] == b">"
        for s in (2, 3, 1023, 1024):
            if f"> opens {s}" in at:
                assert raw[s * S - 1:s * S + 1] == b"\n>", (variant, s)
            elif f"> in sequence {s}" in at:
                assert raw[s * S:s * S + 1] == b">" and raw[s * S - 1:s * S] in (b"A", b"C", b"G", b"T"), (variant, s)
        if variant == 0:
            assert sorted(k for k in at if k.startswith("> ")) == ["> in sequence 1024", "> in sequence 3", "> opens 1023", "> opens 2"]
        else:
            assert sorted(k for k in at if k.startswith("> ")) == ["> in sequence 1023", "> in sequence 2", "> opens 3"]
            assert raw[1024 * S - 2:1024 * S + 2] in (b"A\r\n>", b"C\r\n>", b"G\r\n>", b"T\r\n>", b"N\r\n>", b"a\r\n>", b"c\r\n>", b"g\r\n>", b"t\r\n>")
        # the long header: from inside thread 254's pair of super-tiles to inside thread 256's, thread 255's whole pair in it
        h0, h1 = lv.LONG_HEADER
        assert raw[h0 - 1:h0 + 1] == b"\n>" and raw[h1:h1 + 1] == b"\n" and b"\n" not in raw[h0:h1] and h1 - h0 >= 3 * S
        assert h0 // S // 2 == 254 and h1 // S // 2 == 256 and h0 < 510 * S and 512 * S <= h1
        # workgroup 0 of the compact pass: tiles 0, 4096, 8192, 12288, 16384
        tile = lambda t: raw[max(t * lv.TILE - 1, 0):(t + 1) * lv.TILE]  # noqa: E731  (with the byte in front of it)
        assert tile(0)[:1] == b">" and b"\n>" not in tile(4096) and (b"\n>" in tile(16384)) == (variant == 1)  # header start; in a run
        assert h0 < 8192 * lv.TILE and 8193 * lv.TILE <= h1                      # no kept byte: inside the header
        assert tile(12288).count(b"\n>") == 8
        last = at["records in the last tile"]
        assert 16385 * lv.TILE < last and raw[last:last + 12] == b"\n>a\nACGT\nGG\n" and -(-len(raw) // lv.TILE) == 16386
        want = fasta_ref.parse(raw)
        ids = [raw[r.id_start:r.id_start + min(r.id_len, 12)] for r in want]
        assert ids[:4] == [b"chr0 first", b"s2 x" if variant == 0 else b"s3 x", b"hhhhhh>h\rhhh", b"e0"]
        assert ids[-5:] == ([b"s1023 x"] if variant == 0 else [b"behind crlf"]) + [b"a", b"b", b"c d", b"last"] and len(want) == 16
        assert want[-1].seq.startswith(b"ACG") and want[-2].seq == b"T" and want[-3].seq == b""
        assert want[2].id_len == h1 - h0 - 1 and (want[-5].seq[:2] == b"AC") == (variant == 1)
        assert [len(r.seq) for r in want if raw[r.id_start:r.id_start + 1] == b"e"] == [0, 0, 0]


def test_fasta_many_records_closed_form_equals_the_parse():
    raw, cols, layout = lv.fasta_many_records()
    n_rec = lv.FASTA_MANY_RECORDS
    assert raw.count(b">") == n_rec == len(cols["id_starts"]) and 4 * n_rec <= len(raw) <= 6 * n_rec + 2 * 4200
    for r, kind in lv.REC_LONG.items():
        assert int(cols["seq_lens"][r]) == (65 if kind == 3 else 4097) and r % 1024 in (1, 1023)
    assert {r // 1024 for r in lv.REC_LONG} == {1022, 1023, 1024}
    start = cols["id_starts"] - np.uint64(1)
    for r0, r1 in lv.fasta_record_slices():
        lo, hi = int(start[r0]), int(start[r1]) if r1 < n_rec else len(raw)
        want = fasta_ref.parse(raw[lo:hi])
        assert len(want) == r1 - r0
        assert [r.id_start + lo for r in want] == cols["id_starts"][r0:r1].tolist()
        assert [r.id_len for r in want] == cols["id_lens"][r0:r1].tolist()
        assert [r.seq_len for r in want] == cols["seq_lens"][r0:r1].tolist()
        first = int(cols["seq_starts"][r0])
        assert [r.seq_start + first for r in want] == cols["seq_starts"][r0:r1].tolist()
        piece = fasta_ref.layout(want)
        assert layout[first:first + len(piece) - 64] == piece[:-64]
    assert len(layout) == int(cols["seq_starts"][-1]) + (int(cols["seq_lens"][-1]) + 63) // 64 * 64 + 64 and layout[-64:] == bytes(64)


# ---------------------------------------------------------------- lines
def test_lines_big_plants():
    text = lv.lines_big()
    S = lv.SUPER
    assert len(text) == lv.LINES_BIG
    count = lambda s: text.count(b"\n", s * S, (s + 1) * S)  # noqa: E731
    assert [count(s) for s in (0, 1, 2, 3, 4, 5, 1021, 1022, 1023, 1024)] == [0, 819, 1149, 0, 0, 65536, 65536, 1149, 1, 1]
    assert text[1024 * S - 1:1024 * S + 1] == b"\n\n"
    first, last = lv.lines_spans()
    assert (first <= last).all() and int(last.max()) == len(text)
    singles = set(first[first == last].tolist())
    assert {s * S for s in (0, 1, 2, 3, 1022, 1023, 1024)} | {s * S + S - 1 for s in (0, 1, 2, 3, 1022, 1023)} | {len(text) - 1, len(text)} <= singles
    assert any(a // S // 2 != b // S // 2 for a, b in zip(first.tolist(), last.tolist()))
    assert line_spans_ref.line_span(text, 1024 * S, 1024 * S) == (text.count(b"\n") , text.count(b"\n"), 1024 * S, 1024 * S)
