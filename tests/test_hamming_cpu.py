"""CPU-only: the Hamming search's surface (sassy_hip_search_hamming, Searcher.search_hamming, `search --hamming`) -- what
needs no device: the symbol, every refusal with its code and message before any device work, the loud failure without a
device, the numpy helper against the oracle (the three ties of the issue), the arithmetic header driven by a stand-alone
host program under AddressSanitizer / UBSan, the CLI's parser and row writer on a canned record."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import oracle  # noqa: E402
import hamming_ref as href  # noqa: E402


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
    name = "sassy_hip_search_hamming"
    assert re.search(r"\b" + name + r"\s*\(", hdr)
    assert hasattr(sassy.lib(), name) and name in sassy.EXPORTED_SYMBOLS
    assert re.search(r"fn\s+" + name + r"\s*\(", rust)
    assert re.search(r"#define\s+SASSY_HIP_HAMMING_MAX_ROWS\s+1024", hdr)
    f = sassy.lib().sassy_hip_search_hamming
    assert f.restype is not None and len(f.argtypes) == 9
    names = [r[0] for r in sassy.option_table()]
    assert {"hamming_items", "hamming_records", "hamming_batch"} <= set(names)
    src = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"hamming.hip"' in src


def test_step_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "hamming_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src
    outside = re.sub(r"#if defined\(__HIP_DEVICE_COMPILE__\).*?#else", "", src, flags=re.S)
    assert "__builtin_amdgcn" not in outside


def test_plan_header_is_free_of_hip():
    """csrc/hamming_plan.h, the host's decisions: no HIP header, no searcher, no device builtin, nothing but hamming_step.h."""
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "hamming_plan.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "sassy_SearcherType" not in src
    assert "__builtin_amdgcn" not in src and "__device__" not in src
    assert re.findall(r'#include "([^"]+)"', src) == ["hamming_step.h"]


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal of the issue's table with its code and a message that names the reason, in a child that sees no device:
    a call that got as far as the device would say 'no usable HIP device' instead.  Then valid arguments: that message."""
    code = r'''
import ctypes as C, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
def call(s, pats, text=b"ACGTACGTACGTACGT", k=1, flags=0):
    pp = (C.c_char_p * max(1, len(pats)))(*pats)
    pl = (C.c_size_t * max(1, len(pats)))(*[len(p) for p in pats])
    out = C.c_void_p()
    rc = L.sassy_hip_search_hamming(s._h, pp, pl, len(pats), text, len(text), k, flags, C.byref(out))
    return rc, L.sassy_hip_last_error().decode()
def refused(s, want, word, *a, **kw):
    rc, msg = call(s, *a, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (rc, msg, want, word)
dna = sassy_amd.Searcher("dna", rc=False)
refused(sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang", [b"ACGT"])
refused(sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match", [b"ACGT"])
refused(sassy_amd.Searcher("ascii", rc=True), EUNSUPPORTED, "reverse complement is not defined", [b"ACGT"])
refused(sassy_amd.Searcher("ascii_ci", rc=True), EUNSUPPORTED, "reverse complement is not defined", [b"ACGT"])
refused(dna, EINVAL, "at least one pattern", [])
refused(dna, EINVAL, "empty pattern", [b"ACGT", b""])
refused(sassy_amd.Searcher("iupac", rc=True), EINVAL, "not valid IUPAC", [b"ACGT", b"ACQT"])
refused(dna, EINVAL, "2^31", [b"ACGT"], k=0x80000000)
refused(dna, EUNSUPPORTED, "at most 1024 rows", [b"ACGT", b"A" * 1025])
refused(sassy_amd.Searcher("ascii", rc=False), EUNSUPPORTED, "distinct bytes", [bytes(range(65))])
refused(sassy_amd.Searcher("ascii_ci", rc=False), EUNSUPPORTED, "distinct bytes", [bytes(range(20, 120))])
for flags in (sassy_amd.ALL_MINIMA, sassy_amd.LINE_SPANS, 1 << 20):
    refused(dna, EINVAL, "search_hamming takes", [b"ACGT"], flags=flags)
assert L.sassy_hip_search_hamming(None, None, None, 0, None, 0, 0, 0, None) == EINVAL
# ascii_ci folds before it counts: 52 letters are 26 slots, and the longest allowed pattern passes the argument checks
for s, pats, k in ((sassy_amd.Searcher("ascii_ci", rc=False), [bytes(range(65, 91)) + bytes(range(97, 123))], 1), (dna, [b"A" * 1024], 0x7FFFFFFF),
                   (sassy_amd.Searcher("ascii", rc=False), [bytes(range(64)), bytes(range(64, 128))], 0)):
    rc, msg = call(s, pats, k=k)
    assert rc == ENODEVICE and "no usable HIP device" in msg, (rc, msg)
try:
    dna.search_hamming(sassy_amd.parse_classes(b"a[bc]"), b"abc", 0)
except sassy_amd.SassyHipError as e:
    assert "ClassPattern" in str(e), e
else:
    raise SystemExit(3)
try:
    dna.search_hamming([b"ACGT", sassy_amd.parse_classes(b"a[bc]")], b"abc", 0)
except sassy_amd.SassyHipError as e:
    assert "ClassPattern" in str(e), e
else:
    raise SystemExit(4)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_no_device_fails_loudly(sassy):
    code = (
        "import sassy_amd\n"
        "assert sassy_amd.device_count() == 0\n"
        "for alphabet, rc in (('dna', True), ('iupac', False), ('ascii', False), ('ascii_ci', False)):\n"
        "    s = sassy_amd.Searcher(alphabet, rc=rc)\n"
        "    for pats in (b'ACGT', [b'ACGT', b'AC']):\n"
        "        for wt in (False, True):\n"
        "            try:\n"
        "                s.search_hamming(pats, b'ACGTACGTACGT', 1, without_trace=wt)\n"
        "            except sassy_amd.SassyHipError as e:\n"
        "                assert 'no usable HIP device' in str(e), e\n"
        "            else:\n"
        "                raise AssertionError('no SassyHipError')\n"
        "print('ok')\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


# ---------------------------------------------------------------- the helper against the oracle
ALPHABETS = {"dna": b"ACGT", "iupac": b"ACGTNRYKM", "ascii": b"abcdeAB _"}


def _case(rng, profile, m, n):
    letters = ALPHABETS[profile]
    text = bytearray(rng.choice(letters) for _ in range(n))
    pattern = bytes(rng.choice(letters[:4] if profile != "ascii" else letters) for _ in range(m))
    for _ in range(6):  # plants with a few substitutions
        at = rng.randrange(0, n - m + 1)
        text[at:at + m] = pattern
        for _ in range(rng.randrange(0, 4)):
            text[at + rng.randrange(m)] = rng.choice(letters)
    return pattern, bytes(text)


@pytest.mark.parametrize("profile", ["dna", "iupac", "ascii"])
def test_edit_distance_never_exceeds_the_mismatch_count(profile):
    """oracle.last_row(...)[s + m] <= H(s) for every start: the substitution-only alignment is one of the DP's paths."""
    rng = random.Random(11)
    for m in (1, 2, 7, 31, 32, 33, 64, 65):
        pattern, text = _case(rng, profile, m, 700)
        h = href.mismatches(profile, pattern, text)
        row = oracle.last_row(profile, pattern, text)
        assert len(h) == len(text) - m + 1
        assert (row[m:] <= h).all(), (profile, m)


@pytest.mark.parametrize("profile", ["dna", "iupac", "ascii"])
def test_k0_hits_are_the_oracles_exact_matches(profile):
    rng = random.Random(12)
    for m in (1, 3, 20, 33, 65):
        pattern, text = _case(rng, profile, m, 900)
        want = sorted({(x.text_start, x.text_end) for x in oracle.search(profile, pattern, text, 0, all_minima=True)})
        got = [(x.text_start, x.text_end) for x in href.expected(profile, pattern, text, 0)]
        assert got == want and (m > 20 or got), (profile, m)


@pytest.mark.parametrize("profile", ["dna", "iupac"])
def test_minus_records_are_the_oracles_indel_free_rc_records(profile):
    """The minus-strand convention (forward coordinates, cigar in pattern direction): every '-' record of
    oracle.search_modes(rc=True) that holds no indel is one of the helper's '-' records, field for field."""
    rng = random.Random(13)
    seen = 0
    for m in (8, 21, 40):
        for _ in range(6):
            pattern, text = _case(rng, profile, m, 600)
            rcp = oracle.reverse_complement(profile, pattern)
            t = bytearray(text)
            for _ in range(4):  # plants of the other strand, too
                at = rng.randrange(0, len(t) - m + 1)
                t[at:at + m] = rcp
                t[at + rng.randrange(m)] = rng.choice(b"ACGT")
            text = bytes(t)
            k = 3
            mine = {href.key(x) for x in href.expected(profile, pattern, text, k, rc=True) if x.strand == "-"}
            for x in oracle.search_modes(profile, pattern, text, k, rc=True, all_minima=True):
                if x.strand == "-" and "I" not in x.cigar and "D" not in x.cigar:
                    assert href.key(x) in mine, x
                    seen += 1
    assert seen > 50


def test_relation_rows_are_the_documented_relations():
    for p in b"ACGTacgtN":
        row = href.relation_row("dna", p)
        assert [bool(row[t]) for t in range(256)] == [((p >> 1) & 3) == ((t >> 1) & 3) for t in range(256)]
    assert href.relation_row("iupac", ord("N"))[ord("A")] and not href.relation_row("iupac", ord("R"))[ord("C")]
    assert href.relation_row("ascii", ord("a")).sum() == 1
    row = href.relation_row("ascii_ci", ord("Q"))
    assert row[ord("q")] and row[ord("Q")] and row.sum() == 2
    assert href.relation_row("ascii_ci", ord("["))[ord("[")] and href.relation_row("ascii_ci", ord("[")).sum() == 1


def test_helper_n_rule_and_order():
    text = b"ACGTNACGTNNCGT"
    got = href.expected("iupac", [b"GTAC", b"ACGT"], text, 2, rc=True, max_n_frac=0.25)
    assert [href.key(x)[:1] + (x.strand,) for x in got] == sorted(href.key(x)[:1] + (x.strand,) for x in got)
    for x in got:
        assert text[x.text_start:x.text_end].count(b"N") <= 1
    assert any(text[x.text_start:x.text_end].count(b"N") == 1 for x in got)
    assert len(href.expected("iupac", [b"GTAC", b"ACGT"], text, 2, rc=True)) > len(got)


# ---------------------------------------------------------------- the arithmetic header, on the host
def test_step_header_against_brute_force_under_sanitizers(tmp_path):
    """tests/c/hamming_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: hit masks over random slot masks for m in 1 .. 200, 256, 257, 1024 and every k of the
    issue's list, every counter width that can hold k, the N count, the position mask, cost / N count / cigar per hit."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hamming_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "hamming_step_driver.cc")])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
        assert int(fields["cases"]) == 203 * 17 and int(fields["emits"]) == 203 * 8
        assert 0.2 * 64 * int(fields["cases"]) < int(fields["hits"]) < 0.9 * 64 * int(fields["cases"])  # both sides of the threshold


# ---------------------------------------------------------------- CLI
def test_cli_parses_hamming_and_formats_a_canned_record(sassy, capsys):
    from sassy_amd import cli
    text = b"GGACGTACGTTT"
    s = sassy.Searcher("dna", rc=True)
    m = sassy.Match(pattern_idx=1, text_idx=0, text_start=2, text_end=10, pattern_start=0, pattern_end=8, cost=1, strand="+",
                    cigar="3=1X4=")
    rows = cli.hamming_rows(s, [("p0", b"AAAA"), ("p1", b"ACGAACGT")], "rec1", text, [m])
    assert rows == ["p1\trec1\t1\t+\t2\t10\tACGTACGT\t3=1X4=\n"]
    # the parser: --hamming is a flag of `search`, and refuses --best
    with pytest.raises(SystemExit):
        cli.main(["search", "--hamming", "--best", "-p", "ACGT", "-k", "1", "nofile.fa"])
    assert "--hamming takes neither" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["filter", "--hamming", "-p", "ACGT", "-k", "1", "nofile.fa"])
