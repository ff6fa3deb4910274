"""CPU-only checks for best_matches (sassy_hip_best_matches, Searcher.best_matches, `search --best`):

- the claim its device path rests on: the rightmost end position at which a pair's last row attains its
  global minimum c <= k is an end position the report rule reports, with that cost -- so one candidate per text can go
  to the traceback with no sort and no report rule.  Checked against the oracle for Dna and Iupac, one and both strands,
  with and without overhang, on random pairs with planted occurrences and on low-complexity pairs (long plateaus);
- the expected-value helper (tests/helpers/best_matches_ref.py) on hand-written cases, one tie rule each;
- the surface: header, exported symbols, Rust shim, CLI help, the argument errors that come before any device work."""
import os
import random
import re
import subprocess
import sys

import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import best_matches_ref as ref  # noqa: E402

ALPHA = 0.5


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, edits, alphabet=b"ACGT"):
    s = bytearray(s)
    for _ in range(edits):
        t, p = rng.randrange(3), rng.randrange(len(s))
        if t == 0:
            s[p] = rng.choice(alphabet)
        elif t == 1:
            s.insert(p, rng.choice(alphabet))
        elif len(s) > 1:
            del s[p]
    return bytes(s)


def random_pairs(rng, n, profile):
    """(pattern, text, k): random text, the pattern planted (mutated) zero to two times, anywhere -- the two ends of the text
    included, cut off there for the overhang searches."""
    letters = b"ACGT" if profile == "dna" else b"ACGTACGTACGTNRYSW"
    out = []
    for _ in range(n):
        m = rng.randrange(8, 41)
        k = rng.randrange(0, m // 3 + 1)
        p = rand_seq(rng, m)
        text = bytearray(rand_seq(rng, rng.randrange(m, 260), letters))
        for _ in range(rng.randrange(0, 3)):
            ins = mutate(rng, p, rng.randrange(0, k + 2))
            if rng.random() < 0.5:
                ins = oracle.reverse_complement(profile, ins)
            cut = rng.randrange(0, len(ins) // 2) if rng.random() < 0.3 else 0
            where = rng.choice(["front", "back", "inside"])
            if where == "front":
                ins = ins[cut:]
                text[0:len(ins)] = ins
            elif where == "back":
                ins = ins[:len(ins) - cut]
                text[len(text) - len(ins):] = ins
            else:
                at = rng.randrange(0, max(1, len(text) - len(ins)))
                text[at:at + len(ins)] = ins
        out.append((p, bytes(text), k))
    return out


def low_complexity_pairs(rng, profile):
    """Poly-A, microsatellites, N runs (Iupac): plateaus of equal cost, ties between end positions; k up to m / 3."""
    out = []
    units = [b"A", b"AC", b"AT", b"ACG", b"AAT", b"CAG", b"ACGT", b"GATA"]
    for unit in units:
        for m in (9, 12, 24, 33):
            p = (unit * m)[:m]
            for k in sorted({0, 1, m // 6, m // 3}):
                for n in (m - 2, m, m + 5, 3 * m, 150):
                    if n < 1:
                        continue
                    t = (unit * n)[:n]
                    out.append((p, t, k))
                    out.append((p, rand_seq(rng, 7) + t + rand_seq(rng, 5), k))
                    out.append((mutate(rng, p, 1), t[:n // 2] + rand_seq(rng, 2) + t[n // 2:], k))
                    if profile == "iupac":
                        half = n // 2
                        out.append((p, t[:half] + b"N" * rng.randrange(1, m + 4) + t[half:], k))
                        out.append((p[:m // 2] + b"N" + p[m // 2 + 1:], b"N" * 6 + t + b"N" * (m // 2), k))
    return out


def scan_end(match, text_len, m):
    """The end position in the strand's scan coordinates (the Rc strand is scanned on the reversed text), virtual columns
    behind the text's end included."""
    inside = text_len - match.text_start if match.strand == "-" else match.text_end
    return inside + (m - match.pattern_end)


def rightmost_minimum_is_reported(profile, rc, overhang, p, t, k):
    """Returns (checked strands with a match, strands checked)."""
    m = len(p)
    found = 0
    if overhang:
        every = oracle.search_overhang(profile, p, t, k, ALPHA, rc=rc, all_minima=True)
        reported = oracle.search_overhang(profile, p, t, k, ALPHA, rc=rc)
    else:
        reported = oracle.search(profile, p, t, k, rc=rc)
    strands = ("+", "-") if rc else ("+",)
    for strand in strands:
        if overhang:
            ends = [(scan_end(x, len(t), m), x.cost) for x in every if x.strand == strand]
        else:
            pattern, text = (oracle.complement(profile, p), t[::-1]) if strand == "-" else (p, t)
            row = oracle.last_row(profile, pattern, text)
            ends = [(int(e), int(c)) for e, c in enumerate(row) if c <= k]
        if not ends:
            assert not [x for x in reported if x.strand == strand], (profile, rc, overhang, p, t, k, strand)
            continue
        c = min(cost for _, cost in ends)
        e = max(end for end, cost in ends if cost == c)
        rep = {(scan_end(x, len(t), m), x.cost) for x in reported if x.strand == strand}
        assert (e, c) in rep, (profile, rc, overhang, p, t, k, strand, (e, c), sorted(rep))
        found += 1
    return found, len(strands)


# (overhang is defined through the Iupac profile: its virtual columns are 'N', which a Dna searcher cannot trace -- the
# reference panics there and the oracle's traceback fails -- so the overhang configurations are the Iupac ones)
CONFIGS = [("dna", False, False), ("dna", True, False), ("iupac", False, False), ("iupac", True, False), ("iupac", False, True),
           ("iupac", True, True)]


@pytest.mark.parametrize("profile,rc,overhang", CONFIGS, ids=["-".join((p, "rc" if r else "fwd", "overhang" if o else "plain")) for p, r, o in CONFIGS])
def test_rightmost_global_minimum_is_a_reported_end(profile, rc, overhang):
    """Every case is checked: no pair is skipped, a pair without an end position of cost <= k must have no report."""
    rng = random.Random(20240 + 7 * (profile == "dna") + 2 * rc + overhang)
    pairs = random_pairs(rng, 600, profile) + low_complexity_pairs(rng, profile)
    assert len(pairs) >= 600 + 300
    found = total = 0
    for p, t, k in pairs:
        f, n = rightmost_minimum_is_reported(profile, rc, overhang, p, t, k)
        found += f
        total += n
    print(profile, rc, overhang, "pairs", len(pairs), "strand passes", total, "with a match", found)
    assert found >= total // 4  # (the planted occurrences and the repeats do match)


def test_random_pairs_are_at_least_two_thousand():
    rng = random.Random(1)
    assert len(CONFIGS) * 600 >= 2000 and len(random_pairs(rng, 600, "iupac")) == 600


# ---- the expected-value helper, one tie rule per case ----
M = oracle.Match


def rec(pattern_idx, ts, te, cost, strand, ps=0, pe=8, cigar="8="):
    return M(pattern_idx, ts, te, ps, pe, cost, strand, cigar)


def test_helper_lowest_cost_wins_whatever_the_rest():
    a, b = rec(5, 0, 8, 1, "-"), rec(0, 30, 38, 2, "+")
    assert ref.best_of([b, a]) is a and ref.best_of([a, b]) is a


def test_helper_tie_on_cost_across_patterns_lowest_index():
    a, b = rec(3, 10, 18, 1, "+"), rec(2, 0, 8, 1, "-")
    assert ref.best_of([a, b]) is b


def test_helper_forward_before_rc():
    a, b = rec(2, 0, 8, 1, "-"), rec(2, 40, 48, 1, "+")
    assert ref.best_of([a, b]) is b and ref.best_of([b, a]) is b


def test_helper_two_equal_ends_forward_rightmost_is_largest_text_end():
    a, b = rec(2, 0, 8, 1, "+"), rec(2, 40, 48, 1, "+")
    assert ref.best_of([a, b]) is b and ref.best_of([b, a]) is b


def test_helper_two_equal_ends_rc_rightmost_in_scan_is_smallest_text_start():
    a, b = rec(2, 0, 8, 1, "-"), rec(2, 40, 48, 1, "-")
    assert ref.best_of([a, b]) is a and ref.best_of([b, a]) is a


def test_helper_overhang_behind_the_end_the_further_one_is_right():
    a, b = rec(2, 44, 50, 1, "+", pe=6), rec(2, 45, 50, 1, "+", pe=5)
    assert ref.best_of([a, b]) is b


def test_helper_expected_on_an_oracle_case():
    """Two occurrences of one barcode at equal cost in a read, on each strand: the rightmost in scan direction."""
    p = b"ACGGTCATTGCA"
    filler = b"TTTTTTTTTT"
    for strand_first, profile in ((False, "iupac"), (True, "iupac"), (False, "dna")):
        occ = oracle.reverse_complement(profile, p) if strand_first else p
        t = filler + occ + filler + occ + filler
        got = ref.expected(lambda a, b: oracle.search(profile, a, b, 1, rc=True), [b"GGGGGGGGGGGG", p], [b"", t, filler])
        assert len(got) == 1
        ti, pi, ts, te, ps, pe, cost, strand, cigar = got[0]
        assert (ti, pi, cost, ps, pe, cigar) == (1, 1, 0, 0, 12, "12=")
        if strand_first:
            assert (strand, ts, te) == ("-", 10, 22)      # the leftmost in the text: the rightmost of the reversed scan
        else:
            assert (strand, ts, te) == ("+", 32, 44)
        assert ref.expected_fast(profile, [b"GGGGGGGGGGGG", p], [b"", t, filler], 1, True, threads=2) == got
        assert ref.without_trace(got[0])[2:5] == ((10, (1 << 64) - 1, (1 << 64) - 1) if strand_first else ((1 << 64) - 1, 44, (1 << 64) - 1))


# ---- surface ----
@pytest.fixture(scope="module")
def sassy():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


def test_symbol_is_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    name = "sassy_hip_best_matches"
    assert re.search(r"\b" + name + r"\s*\(", hdr)
    assert hasattr(sassy.lib(), name)
    assert name in sassy.EXPORTED_SYMBOLS
    assert re.search(r"fn\s+" + name + r"\s*\(", rust) and re.search(r"pub fn best_matches\s*\(", rust)
    assert "best_match_device" in [r[0] for r in sassy.option_table()]
    assert callable(sassy.Searcher.best_matches)


def test_cli_help_shows_best():
    p = subprocess.run([sys.executable, "-m", "sassy_amd", "search", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "--best" in p.stdout, p.stdout + p.stderr


def test_argument_errors_come_before_any_device_work(sassy):
    """k = 255, a foreign flag, Ascii with rc and null arguments fail whether or not the box has a device (the child sees
    none); valid arguments then ask for the device and fail loudly, on both settings of best_match_device."""
    code = (
        "import ctypes as C, sassy_amd\n"
        "L = sassy_amd.lib()\n"
        "s = sassy_amd.Searcher('iupac', rc=True)\n"
        "pats, texts = [b'ACGTACGTAC', b'TTGACCATGA'], [b'ACGTACGTACGT', b'GGGG', b'']\n"
        "pp = (C.c_char_p * 2)(*pats); pl = (C.c_size_t * 2)(10, 10)\n"
        "tp = (C.c_char_p * 3)(*texts); tp = C.cast(tp, C.POINTER(C.c_void_p)); tl = (C.c_size_t * 3)(12, 4, 0)\n"
        "out = C.c_void_p()\n"
        "def err():\n"
        "    return L.sassy_hip_last_error().decode()\n"
        "for k, flags in ((255, 0), (1, sassy_amd.ALL_MINIMA), (1, 8), (1, 64)):\n"
        "    assert L.sassy_hip_best_matches(s._h, pp, pl, 2, tp, tl, 3, k, flags, C.byref(out)) == -1, (k, flags, err())\n"
        "    assert 'no usable HIP device' not in err(), err()\n"
        "assert L.sassy_hip_best_matches(None, pp, pl, 2, tp, tl, 3, 1, 0, C.byref(out)) == -1\n"
        "assert L.sassy_hip_best_matches(s._h, pp, pl, 2, tp, tl, 3, 1, 0, None) == -1\n"
        "a = sassy_amd.Searcher('ascii', rc=True)\n"
        "assert L.sassy_hip_best_matches(a._h, pp, pl, 2, tp, tl, 3, 1, 0, C.byref(out)) == -3 and 'ascii' in err(), err()\n"
        "for dev in (1, 0):\n"
        "    s.set_option('best_match_device', dev)\n"
        "    for flags in (0, sassy_amd.WITHOUT_TRACE):\n"
        "        assert L.sassy_hip_best_matches(s._h, pp, pl, 2, tp, tl, 3, 1, flags, C.byref(out)) == -2 and 'no usable HIP device' in err(), err()\n"
        "    for tx in (texts, sassy_amd.TextBatch.from_list(texts)):\n"
        "        try:\n            s.best_matches(pats, tx, 1)\n        except sassy_amd.SassyHipError as e:\n            assert 'no usable HIP device' in str(e), e\n        else:\n            raise SystemExit(3)\n"
        "try:\n    s.best_matches(pats, texts, 300)\nexcept sassy_amd.SassyHipError as e:\n    assert 'k must be <= 254' in str(e), e\nelse:\n    raise SystemExit(4)\n"
        "print('ok')\n"
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
