"""CPU-only: the batch Hamming calls' surface (sassy_hip_search_hamming_many, sassy_hip_hamming_best_pattern, the Python
methods, `search --hamming` over a batch, `demux`) -- what needs no device: the symbols, every refusal with its code and
message before any device work, the loud failure without a device, the batch arithmetic of hamming_step.h driven by a
stand-alone host program under AddressSanitizer / UBSan, the helper on a hand-written case, the CLI's parser and row writers."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import hamming_many_ref as mref  # noqa: E402

NAMES = ("sassy_hip_search_hamming_many", "sassy_hip_hamming_best_pattern")


@pytest.fixture(scope="module")
def sassy():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


def test_symbols_are_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(sassy.lib(), name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", rust), name
        assert re.search(r"pub fn\s+" + name[len("sassy_hip_"):] + r"\s*\(", rust), name
    L = sassy.lib()
    assert L.sassy_hip_search_hamming_many.restype is not None and len(L.sassy_hip_search_hamming_many.argtypes) == 10
    assert L.sassy_hip_hamming_best_pattern.restype is not None and len(L.sassy_hip_hamming_best_pattern.argtypes) == 13
    assert "hamming_many_batch" in [r[0] for r in sassy.option_table()]
    assert hasattr(sassy.Searcher, "search_hamming_many") and hasattr(sassy.Searcher, "hamming_best_pattern")


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal of the issue's list, for both entry points, with its code and a message that names the reason, in a
    child that sees no device: a call that got as far as the device would say 'no usable HIP device' instead.  Then valid
    arguments: that message.  n_texts == 0 is an empty result without a device."""
    code = r'''
import ctypes as C, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
def call(which, s, pats, texts=(b"ACGTACGTACGTACGT", b"", b"ACG"), k=1, flags=0, lens=None):
    pp = (C.c_char_p * max(1, len(pats)))(*pats)
    pl = (C.c_size_t * max(1, len(pats)))(*[len(p) for p in pats])
    keep = [C.create_string_buffer(t, max(1, len(t))) for t in texts]
    tp = (C.c_void_p * max(1, len(texts)))(*[C.addressof(b) for b in keep])
    tl = (C.c_size_t * max(1, len(texts)))(*(lens if lens is not None else [len(t) for t in texts]))
    n = len(texts)
    if which == "many":
        out = C.c_void_p()
        rc = L.sassy_hip_search_hamming_many(s._h, pp, pl, len(pats), tp, tl, n, k, flags, C.byref(out))
        if rc == 0:
            assert L.sassy_hip_result_len(out) == 0
            L.sassy_hip_result_free(out)
    else:
        cost = (C.c_uint8 * max(1, n))()
        pat = (C.c_uint32 * max(1, n))()
        strand = (C.c_uint8 * max(1, n))()
        start = (C.c_uint64 * max(1, n))()
        rc = L.sassy_hip_hamming_best_pattern(s._h, pp, pl, len(pats), tp, tl, n, k, flags, cost, pat, strand, start)
    return rc, L.sassy_hip_last_error().decode()
def refused(which, s, want, word, *a, **kw):
    rc, msg = call(which, s, *a, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (which, rc, msg, want, word)
dna = sassy_amd.Searcher("dna", rc=False)
for which in ("many", "best"):
    refused(which, sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang", [b"ACGT"])
    refused(which, sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match", [b"ACGT"])
    refused(which, sassy_amd.Searcher("ascii", rc=True), EUNSUPPORTED, "reverse complement is not defined", [b"ACGT"])
    refused(which, sassy_amd.Searcher("ascii_ci", rc=True), EUNSUPPORTED, "reverse complement is not defined", [b"ACGT"])
    refused(which, dna, EINVAL, "at least one pattern", [])
    refused(which, dna, EINVAL, "empty pattern", [b"ACGT", b""])
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, "not valid IUPAC", [b"ACGT", b"ACQT"])
    refused(which, dna, EUNSUPPORTED, "at most 1024 rows", [b"ACGT", b"A" * 1025])
    refused(which, sassy_amd.Searcher("ascii", rc=False), EUNSUPPORTED, "distinct bytes", [bytes(range(65))])
    refused(which, sassy_amd.Searcher("ascii_ci", rc=False), EUNSUPPORTED, "distinct bytes", [bytes(range(20, 120))])
    for flags in (sassy_amd.TEXT_ON_DEVICE, sassy_amd.ALL_MINIMA, sassy_amd.LINE_SPANS, 1 << 20):
        refused(which, dna, EINVAL, "host texts only", [b"ACGT"], flags=flags)
refused("many", dna, EINVAL, "2^31", [b"ACGT"], k=0x80000000)
refused("best", dna, EINVAL, "k must be <= 254", [b"ACGT"], k=255)
refused("best", dna, EINVAL, "host texts only", [b"ACGT"], flags=sassy_amd.WITHOUT_TRACE)
refused("best", dna, EUNSUPPORTED, "shorter than 2^32 bytes", [b"ACGT"], texts=(b"ACGT", b"ACGT"), lens=[4, 1 << 32])
# null pointers
assert L.sassy_hip_search_hamming_many(None, None, None, 0, None, None, 0, 0, 0, None) == EINVAL
assert L.sassy_hip_hamming_best_pattern(None, None, None, 0, None, None, 0, 0, 0, None, None, None, None) == EINVAL
one = (C.c_char_p * 1)(b"ACGT"); onel = (C.c_size_t * 1)(4); out = C.c_void_p()
assert L.sassy_hip_search_hamming_many(dna._h, one, onel, 1, None, None, 2, 1, 0, C.byref(out)) == EINVAL
assert "must not be null" in L.sassy_hip_last_error().decode()
assert L.sassy_hip_search_hamming_many(dna._h, one, onel, 1, None, None, 0, 1, 0, None) == EINVAL
assert L.sassy_hip_hamming_best_pattern(dna._h, one, onel, 1, (C.c_void_p * 1)(), (C.c_size_t * 1)(4), 1, 1, 0, None, None, None, None) == EINVAL
assert "must not be null" in L.sassy_hip_last_error().decode()
# n_texts == 0: an empty result, 0 -- and no device is asked for
for which in ("many", "best"):
    rc, msg = call(which, dna, [b"ACGT"], texts=())
    assert rc == 0, (which, rc, msg)
assert dna.search_hamming_many([b"ACGT"], [], 1) == []
assert [len(a) for a in dna.hamming_best_pattern([b"ACGT"], [], 1)] == [0, 0, 0, 0]
# valid arguments get as far as the device; the optional outputs may be NULL
for which, s, pats, k in (("many", sassy_amd.Searcher("ascii_ci", rc=False), [bytes(range(65, 91)) + bytes(range(97, 123))], 1),
                          ("many", dna, [b"A" * 1024], 0x7FFFFFFF), ("best", dna, [b"A" * 1024], 254),
                          ("many", sassy_amd.Searcher("dna", rc=True), [b"ACGT"], 1),
                          ("best", sassy_amd.Searcher("ascii", rc=False), [bytes(range(64)), bytes(range(64, 128))], 0)):
    rc, msg = call(which, s, pats, k=k)
    assert rc == ENODEVICE and "no usable HIP device" in msg, (which, rc, msg)
tl = (C.c_size_t * 1)(4); keep = C.create_string_buffer(b"ACGT"); tp = (C.c_void_p * 1)(C.addressof(keep)); cost = (C.c_uint8 * 1)()
assert L.sassy_hip_hamming_best_pattern(dna._h, one, onel, 1, tp, tl, 1, 1, 0, cost, None, None, None) == ENODEVICE
for method in ("search_hamming_many", "hamming_best_pattern"):
    for pats in (sassy_amd.parse_classes(b"a[bc]"), [b"ACGT", sassy_amd.parse_classes(b"a[bc]")]):
        try:
            getattr(dna, method)(pats, [b"abc"], 0)
        except sassy_amd.SassyHipError as e:
            assert "ClassPattern" in str(e), e
        else:
            raise SystemExit(3)
    try:
        getattr(dna, method)([b"ACGT"], [b"ACGTACGT", b""], 1)
    except sassy_amd.SassyHipError as e:
        assert "no usable HIP device" in str(e), e
    else:
        raise SystemExit(4)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_refusals_are_one_function():
    """The checks are factored out, not copied: the single-text entry point and the batch entry points call one refusals
    function, which ends in the open-tickets check (tests/test_gpu_hamming_many.py opens a ticket)."""
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "hamming.hip")).read()
    body = src[src.index("\nint hamming_refusals("):]
    body = body[:body.index("\n}\n")]
    assert "SASSY_NO_TICKETS(s);" in body and "only_best_match" in body and "overhang" in body
    assert src.count("hamming_refusals(s, patterns, pattern_lens, n_patterns, k,") == 3  # the single-text call, the two batch calls
    assert src.count("only_best_match is not supported") == 1 and src.count("SASSY_NO_TICKETS") == 1


def test_batch_arithmetic_against_brute_force_under_sanitizers(tmp_path):
    """tests/c/hamming_many_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: the per-text valid mask for rem in {0, 1, m-1, m, m+1, 63, 64, 65, m+63, m+64, saturated} x
    m in {1, 2, 63, 64, 65, 1024}, the block-to-text lookup over start tables with empty texts first, last and in runs, the
    min-cost narrowing for 2, 4, 8 and 11 planes."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hamming_many_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "hamming_many_step_driver.cc")])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
        assert int(fields["masks"]) >= 6 * 11 and int(fields["lookups"]) > 1000
        assert int(fields["minima"]) == 4 * 400 * (7 + 2)


def test_step_header_stays_free_of_hip():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "hamming_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src
    for name in ("ham_valid_mask_rem", "ham_rem", "ham_text_of", "ham_min_cost", "ham_count"):
        assert re.search(r"\b" + name + r"\s*\(", src), name


# ---------------------------------------------------------------- the helper, on a case written out by hand
def test_helper_on_a_hand_written_case():
    pats = [b"ACGT", b"GG"]
    texts = [b"ACGTAGGT", b"", b"CC", b"TTACGA"]
    # k = 1, both strands.  ACGT is its own reverse complement; GG's is CC.
    #   text 0 "ACGTAGGT": ACGT at 0 (0 mismatches), AGGT at 4 (1); GG at 5 (0), at 1 "CG", 2 "GT", 4 "AG" and 6 "GT" (1);
    #           CC: "AC" 0, "CG" 1 (1)
    #   text 2 "CC": GG '-' at 0 (0)
    #   text 3 "TTACGA": ACGA at 2 (1); GG: "CG" 3, "GA" 4 (1); CC: "AC" 2, "CG" 3 (1)
    want = [
        (0, 0, "+", 0, 0, "4="), (0, 0, "+", 4, 1, "1=1X2="), (3, 0, "+", 2, 1, "3=1X"),
        (0, 0, "-", 0, 0, "4="), (0, 0, "-", 4, 1, "2=1X1="), (3, 0, "-", 2, 1, "1X3="),
        (0, 1, "+", 1, 1, "1X1="), (0, 1, "+", 2, 1, "1=1X"), (0, 1, "+", 4, 1, "1X1="), (0, 1, "+", 5, 0, "2="), (0, 1, "+", 6, 1, "1=1X"), (3, 1, "+", 3, 1, "1X1="), (3, 1, "+", 4, 1, "1=1X"),
        (0, 1, "-", 0, 1, "1=1X"), (0, 1, "-", 1, 1, "1X1="), (2, 1, "-", 0, 0, "2="), (3, 1, "-", 2, 1, "1=1X"), (3, 1, "-", 3, 1, "1X1="),
    ]
    got = mref.expected_many("dna", pats, texts, 1, rc=True)
    assert [(t, x.pattern_idx, x.strand, x.text_start, x.cost, x.cigar) for t, x in got] == want
    assert all(x.text_end == x.text_start + len(pats[x.pattern_idx]) and x.pattern_start == 0 for _, x in got)
    # the best per text: text 0 has two records of cost 0 -- pattern 0 '+' wins over pattern 0 '-' and pattern 1; text 1 has
    # none; text 2 its only record; text 3 five of cost 1 -- pattern 0 '+'
    assert mref.expected_best("dna", pats, texts, 1, rc=True) == [
        (0, 0, 0, 0), (mref.NO_MATCH, mref.NO_PATTERN, 0, mref.NO_START), (0, 1, 1, 0), (1, 0, 0, 2)]
    # leftmost on a tie of everything else
    assert mref.expected_best("dna", [b"GG"], [b"AGGTGG"], 0) == [(0, 0, 0, 1)]
    assert mref.expected_best("dna", [b"GG"], [b"AGGTGG"], 0, rc=True) == [(0, 0, 0, 1)]
    assert mref.expected_many("dna", pats, [], 1) == [] and mref.expected_best("dna", pats, [], 1) == []


# ---------------------------------------------------------------- CLI
def test_cli_demux_parser_and_row_writer(sassy, capsys):
    from sassy_amd import cli
    patterns = [("bc1", b"ACGTACGT"), ("bc2", b"TTTTACGT")]
    best = (np.array([1, sassy.NO_MATCH, 0], dtype=np.uint8), np.array([1, 0xFFFFFFFF, 0], dtype=np.uint32),
            np.array([1, 0, 0], dtype=np.uint8), np.array([17, 0xFFFFFFFFFFFFFFFF, 0], dtype=np.uint64))
    rows = cli.demux_rows(patterns, ["r1", "r2", "r3"], best)
    assert rows == ["r1\tbc2\t1\t-\t17\n", "r2\t*\t-1\t*\t-1\n", "r3\tbc1\t0\t+\t0\n"]
    assert cli.DEMUX_HEADER == "text_id\tpat_id\tcost\tstrand\tstart\n"
    with pytest.raises(SystemExit):
        cli.main(["demux", "-p", "ACGT", "-k", "1"])  # no path
    with pytest.raises(SystemExit):
        cli.main(["demux", "-p", "ACGT", "nofile.fa"])  # no k
    with pytest.raises(SystemExit):
        cli.main(["demux", "-p", "ACGT", "-k", "1", "--overhang", "0.5", "nofile.fa"])
    assert "does not take --overhang" in capsys.readouterr().err


def test_cli_batch_rows_keep_the_per_record_order(sassy):
    """hamming_batch_rows on canned records in the batch call's order (pattern, strand, record, start): rows come record by
    record, inside a record in the call's order."""
    from sassy_amd import cli

    class Batch:
        texts = sassy.TextBatch.from_list([b"GGACGTACGTTT", b"ACGAACGT"])

        @staticmethod
        def id(i):
            return ["rec1", "rec2"][i]

    def rec(p, t, start, cost, strand, cigar, m):
        return sassy.Match(pattern_idx=p, text_idx=t, text_start=start, text_end=start + m, pattern_start=0, pattern_end=m, cost=cost,
                           strand=strand, cigar=cigar)

    s = sassy.Searcher("dna", rc=True)
    patterns = [("p0", b"ACGT"), ("p1", b"ACGAACGT")]
    matches = [rec(0, 0, 2, 0, "+", "4=", 4), rec(0, 0, 6, 0, "+", "4=", 4), rec(0, 1, 4, 0, "+", "4=", 4),
               rec(1, 0, 2, 1, "+", "3=1X4=", 8), rec(1, 1, 0, 0, "+", "8=", 8)]
    rows = cli.hamming_batch_rows(s, patterns, Batch, matches)
    assert rows == ["p0\trec1\t0\t+\t2\t6\tACGT\t4=\n", "p0\trec1\t0\t+\t6\t10\tACGT\t4=\n", "p1\trec1\t1\t+\t2\t10\tACGTACGT\t3=1X4=\n",
                    "p0\trec2\t0\t+\t4\t8\tACGT\t4=\n", "p1\trec2\t0\t+\t0\t8\tACGAACGT\t8=\n"]


def test_cli_hamming_still_refuses_best_and_overhang(capsys):
    from sassy_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["search", "--hamming", "--best", "-p", "ACGT", "-k", "1", "nofile.fa"])
    assert "--hamming takes neither" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["search", "--hamming", "--overhang", "0.5", "-p", "ACGT", "-k", "1", "nofile.fa"])
    assert "--hamming takes neither" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["filter", "--hamming", "-p", "ACGT", "-k", "1", "nofile.fa"])
