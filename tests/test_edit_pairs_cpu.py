"""CPU-only: the surface of the all-vs-all edit-distance calls (sassy_hip_edit_pairs, sassy_hip_edit_nearest, the Python
methods, `pairs --edit`) -- what needs no device: the symbols, every refusal with its code and message before any device work,
the loud failure without a device (the |m_a - m_b| > k call included), the arithmetic of edit_pairs_step.h driven by a
stand-alone host program under AddressSanitizer / UBSan, the helper on a hand-written case and against the definition cell by
cell, the CLI's parser and row writers."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import edit_pairs_ref as eref  # noqa: E402
import hamming_pairs_ref as pref  # noqa: E402

NAMES = ("sassy_hip_edit_pairs", "sassy_hip_edit_nearest")
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


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
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    for name in NAMES + ("sassy_hip_edit_pairs_free",):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(sassy.lib(), name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
    for name in NAMES:
        assert re.search(r"pub fn\s+" + name[len("sassy_hip_"):] + r"\s*\(", rust), name
    L = sassy.lib()
    assert L.sassy_hip_edit_pairs.restype is not None and len(L.sassy_hip_edit_pairs.argtypes) == 11
    assert L.sassy_hip_edit_nearest.restype is not None and len(L.sassy_hip_edit_nearest.argtypes) == 13
    assert hasattr(sassy.Searcher, "edit_pairs") and hasattr(sassy.Searcher, "edit_nearest")
    assert re.search(r"typedef\s+sassy_hip_HammingPair\s+sassy_hip_EditPair\s*;", hdr)
    assert re.search(r"\b9: the all-vs-all walk of sassy_hip_edit_pairs", hdr)  # (the stats comment)
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"edit_pairs.hip"' in build and '"edit_pairs_step.h"' in build


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal of both entry points with its code and a message that names the reason, in a child that sees no device:
    a call that got as far as the device would say 'no usable HIP device' instead.  Then valid arguments: that message --
    also where |m_a - m_b| > k, whose empty answer is given only behind the device."""
    code = r'''
import ctypes as C, numpy as np, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
A = b"ACGTACGT" + b"TTTTACGT"
def call(which, s, a=A, n_a=2, m_a=8, b=None, n_b=0, m_b=0, k=1, flags=0, out=True, s_null=False):
    h = None if s_null else s._h
    if which == "pairs":
        o, n = C.c_void_p(), C.c_size_t()
        rc = L.sassy_hip_edit_pairs(h, a, n_a, m_a, b, n_b, m_b, k, flags, C.byref(o) if out else None, C.byref(n) if out else None)
    else:
        cost = np.zeros(max(1, min(n_a, 16)), dtype=np.uint8)
        rc = L.sassy_hip_edit_nearest(h, a, n_a, m_a, b, n_b, m_b, k, flags, cost.ctypes.data if out else None, None, None, None)
    return rc, L.sassy_hip_last_error().decode()
def refused(which, s, want, word, **kw):
    rc, msg = call(which, s, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (which, rc, msg, want, word)
dna = sassy_amd.Searcher("dna", rc=False)
for which in ("pairs", "nearest"):
    # the family's own checks, per list
    refused(which, sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang")
    refused(which, sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match")
    refused(which, sassy_amd.Searcher("ascii", rc=True), EUNSUPPORTED, "reverse complement is not defined")
    refused(which, sassy_amd.Searcher("ascii_ci", rc=True), EUNSUPPORTED, "reverse complement is not defined")
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, "not valid IUPAC", a=b"ACGTACGT" + b"ACQTACGT")
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, "list a)", a=b"ACGTACGT" + b"ACQTACGT")
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, "not valid IUPAC", b=b"ACGTAC1", n_b=1, m_b=7)
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, "list b)", b=b"ACGTAC1", n_b=1, m_b=7)
    refused(which, sassy_amd.Searcher("dna", rc=False).with_max_n_frac(0.2), EUNSUPPORTED, "max_n_frac")
    # the shape
    refused(which, dna, EINVAL, "m_a must be at least 1", m_a=0)
    refused(which, dna, EINVAL, "m_a must be <= 64", a=b"A" * 130, m_a=65)
    refused(which, dna, EINVAL, "m_b must be at least 1", b=A, n_b=2, m_b=0)
    refused(which, dna, EINVAL, "m_b must be <= 64", b=b"A" * 130, n_b=2, m_b=65)
    refused(which, dna, EINVAL, "m_b must be 0 or m_a", m_b=7)       # self mode
    refused(which, dna, EINVAL, "m_b must be 0 or m_a", m_b=65)
    refused(which, dna, EINVAL, "k must be <= 254", k=255)
    refused(which, dna, EINVAL, "k must be <= 254", k=0x80000000)
    refused(which, dna, EINVAL, "at least one sequence", n_a=0)
    refused(which, dna, EINVAL, "n_b is 0", b=A, n_b=0, m_b=8)
    refused(which, dna, EINVAL, "b is NULL", b=None, n_b=2, m_b=8)
    for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.ALL_MINIMA, sassy_amd.TEXT_ON_DEVICE, sassy_amd.TEXT_UNCHANGED, sassy_amd.LINE_SPANS, 1 << 20):
        refused(which, dna, EINVAL, "takes no flags", flags=flags)
    refused(which, dna, EUNSUPPORTED, "2^31 - 1", n_a=1 << 31)
    refused(which, dna, EUNSUPPORTED, "2^31 - 1", b=A, n_b=1 << 31, m_b=8)
    refused(which, dna, EINVAL, "must not be null", out=False)
    refused(which, dna, EINVAL, "must not be null", a=None)
    refused(which, dna, EINVAL, "must not be null", s_null=True)
    # valid arguments get as far as the device: every alphabet, both modes, the limits themselves, lengths of their own,
    # and lengths further apart than k (an empty answer, but only on a machine that has a device)
    for s, kw in ((dna, {}), (dna, dict(m_b=8)), (dna, dict(b=A, n_b=2, m_b=8)), (dna, dict(b=A, n_b=4, m_b=4)), (dna, dict(b=A, n_b=16, m_b=1, k=0)),
                  (sassy_amd.Searcher("dna", rc=True), dict(k=254)), (sassy_amd.Searcher("iupac", rc=True), dict(a=b"ACGTNNRY" * 2)),
                  (sassy_amd.Searcher("ascii", rc=False), {}), (sassy_amd.Searcher("ascii_ci", rc=False), dict(a=b"x" * 128, m_a=64)),
                  (dna, dict(a=b"AC", m_a=1)), (dna, dict(a=b"A" * 64, n_a=1, m_a=64, b=b"C", n_b=1, m_b=1, k=63))):
        rc, msg = call(which, s, **kw)
        assert rc == ENODEVICE and "no usable HIP device" in msg, (which, rc, msg)
# the Python methods: refusals of their own, then the same loud failure; b may have a length of its own
for method in ("edit_pairs", "edit_nearest"):
    f = getattr(dna, method)
    for args, word in ((([b"ACGT", b"ACG"],), "sequence 1 has 3 bytes"), (([b"ACGT"], [b"ACGTA", b"ACGT"]), "sequence 1 has 4 bytes"),
                       (([b"ACGT", sassy_amd.parse_classes(b"a[bc]")],), "ClassPattern"),
                       ((np.zeros((2, 4), dtype=np.int32),), "uint8 array"), (([b"ACGT"], None, 300), "k must be <= 254"),
                       (([],), "needs at least one sequence"), (([b"ACGT"], []), "b holds no sequence"),
                       (([b"A" * 65],), "m_a must be <= 64"), (([b"ACGT"], [b"A" * 65]), "m_b must be <= 64"),
                       (([b"ACGT", b"AAAA"],), "no usable HIP device"), (([b"ACGT"], [b"ACGTA"], 1), "no usable HIP device"),
                       (([b"ACGT"], [b"ACGTACGT"], 1), "no usable HIP device")):
        try:
            f(*args)
        except sassy_amd.SassyHipError as e:
            assert word in str(e), (method, word, e)
        else:
            raise SystemExit(3)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_refusals_are_the_familys_function_and_the_passes_exist_once():
    """No copy of the family's checks: the unit calls hamming_refusals once, for both entry points and both lists, reads
    neither the environment nor holds the strings hamming.hip is pinned to hold once.  No copy of the passes that know
    nothing of the distance either: their kernels stay in hamming_pairs.hip, this unit calls their host functions."""
    src = open(os.path.join(CSRC, "edit_pairs.hip")).read()
    assert src.count("hamming_refusals(") == 1 and src.count("edit_refusals(") == 3 and src.count("family(") == 2  # (once per list)
    body = src[src.index("int edit_refusals("):]
    body = body[:body.index("\n}\n")]
    assert "hamming_refusals(" in body
    for entry in ("int sassy_hip_edit_pairs(", "int sassy_hip_edit_nearest("):
        fn = src[src.index(entry):]
        assert fn.index("edit_refusals(") < fn.index("hamming_call(") < fn.index("edit_lengths_too_far(") < fn.index("edit_survey(")
    assert "only_best_match" not in src and "SASSY_NO_TICKETS" not in src and "getenv" not in src
    assert "asm" not in src
    pairs = open(os.path.join(CSRC, "hamming_pairs.hip")).read()
    internal = open(os.path.join(CSRC, "host_internal.h")).read()
    for kernel in ("pairs_nearest_kernel", "pairs_rows_kernel", "pairs_scan_sums_kernel", "pairs_scan_top_kernel", "pairs_scan_rows_kernel"):
        assert kernel + "(" not in src and kernel + "," not in src and len(re.findall(r"__global__[^;{]*\b" + kernel + r"\(", pairs)) == 1, kernel
    for shared in ("pairs_place_rows(", "pairs_take_records(", "pairs_fold_nearest("):
        assert shared in src and shared in pairs and shared in internal, shared


def test_edit_arithmetic_against_a_plain_dp_under_sanitizers(tmp_path):
    """tests/c/edit_pairs_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: planes, packed codes and the bit-vector column step against a byte-wise DP for every profile
    and every (m_a, m_b) in {1, 2, 31, 32, 33, 63, 64}^2 -- random, equal, matchless and shifted pairs."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    driver = os.path.join(ROOT, "tests", "c", "edit_pairs_step_driver.cc")
    text = open(driver).read()
    assert "int main(" in text and "#include <hip" not in text and "__global__" not in text
    exe = str(tmp_path / "edit_pairs_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, driver])
    pairs_of_lengths = 4 * 7 * 7
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
        assert int(fields["random"]) == 20 * pairs_of_lengths and int(fields["equal"]) == 4 * pairs_of_lengths
        assert int(fields["nomatch"]) == 2 * pairs_of_lengths and int(fields["shifted"]) == 4 * pairs_of_lengths
        # every column's code read back, both ways round: 30 pairs x (m_a + m_b) per pair of lengths
        assert int(fields["codes"]) == 4 * 30 * 2 * 7 * sum((1, 2, 31, 32, 33, 63, 64))


def test_step_header_stays_free_of_hip():
    src = open(os.path.join(CSRC, "edit_pairs_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "getenv" not in src
    assert "__builtin_amdgcn" not in src and "__HIP_DEVICE_COMPILE__" not in src and "asm" not in src
    for name in ("edit_encode_record", "edit_eq", "edit_column", "edit_score", "edit_cost"):
        assert re.search(r"\b" + name + r"\s*[<(]", src), name
    # the kernels and the host share it, with the Hamming pair calls' planes, cells and plan
    unit = open(os.path.join(CSRC, "edit_pairs.hip")).read()
    for name in ("pairs_encode(", "edit_encode_record(", "edit_eq<", "edit_column<", "edit_score<", "pairs_combine(", "pairs_plan(",
                 "pairs_tile_first(", "pairs_visits("):
        assert name in unit, name


# ---------------------------------------------------------------- the helper
def test_helper_on_a_hand_written_case():
    t = eref.as_tuples
    assert t(eref.expected_pairs("dna", eref.HAND_A, eref.HAND_B, eref.HAND_K)) == eref.HAND_PAIRS
    rows = lambda cols: [tuple(int(c[i]) for c in cols) for i in range(len(cols[0]))]
    assert rows(eref.expected_nearest("dna", eref.HAND_A, eref.HAND_B, eref.HAND_K)) == eref.HAND_NEAREST
    # a Hamming-only answer fails this case: CGTA is at Hamming distance 4
    assert t(pref.expected_pairs("dna", eref.HAND_A, eref.HAND_B, eref.HAND_K)) == [(0, 1, 0, 0), (0, 3, 0, 2)]
    # lengths of their own: a base lost, a base gained, further apart than k
    assert t(eref.expected_pairs("dna", [b"ACGT"], [b"ACT", b"CGT", b"GGG"], 1)) == [(0, 0, 0, 1), (0, 1, 0, 1)]
    assert t(eref.expected_pairs("dna", [b"ACGT"], [b"ACGGT", b"TACGT"], 1)) == [(0, 0, 0, 1), (0, 1, 0, 1)]
    assert t(eref.expected_pairs("dna", [b"ACGT"], [b"AC"], 1)) == [] and t(eref.expected_pairs("dna", [b"ACGT"], [b"AC"], 2)) == [(0, 0, 0, 2)]
    # strand 1 and the self-mode triangle: AACG's reverse complement is CGTT, one shift away from ACGT; ACGT is its own
    assert t(eref.expected_pairs("dna", [b"ACGT", b"AACG"], None, 2, rc=True)) == [(0, 0, 1, 0), (0, 1, 0, 2), (0, 1, 1, 2)]
    assert rows(eref.expected_nearest("dna", [b"ACGT", b"AACG"], None, 2, rc=True)) == [(0, 0, 1, 1), (2, 0, 0, 2)]
    # the relation is the family's
    assert t(eref.expected_pairs("iupac", [b"NNNN"], [b"ACG", b"TTT"], 1)) == [(0, 0, 0, 1), (0, 1, 0, 1)]
    assert t(eref.expected_pairs("iupac", [b"NNNN", b"RRYY"], [b"ACGTA", b"AGCTT"], 1)) == [(0, 0, 0, 1), (0, 1, 0, 1), (1, 1, 0, 1)]
    assert t(eref.expected_pairs("ascii_ci", [b"abc"], [b"ABC", b"XBC"], 1)) == [(0, 0, 0, 0), (0, 1, 0, 1)]
    assert t(eref.expected_pairs("ascii_ci", [b"abc"], [b"BC", b"cb"], 1)) == [(0, 0, 0, 1)]
    assert t(eref.expected_pairs("ascii", [b"abc"], [b"BC", b"bc"], 1)) == [(0, 1, 0, 1)]


def test_helper_table_equals_the_definition_cell_by_cell():
    for profile in ("dna", "iupac", "ascii", "ascii_ci"):
        for m_a, m_b in ((1, 1), (3, 9), (9, 3), (12, 12)):
            a, b = eref.related_lists(profile, 7, 9, m_a, m_b, 3, seed=m_a * 31 + m_b)
            e = eref.distances(profile, a, b, False)
            assert e.shape == (7, 9, 1)
            for i in range(7):
                for j in range(9):
                    assert e[i, j, 0] == eref.plain_distance(profile, bytes(a[i]), bytes(b[j])), (profile, m_a, m_b, i, j)


# ---------------------------------------------------------------- CLI
def test_cli_pairs_parser_takes_edit(sassy, capsys, tmp_path):
    from sassy_amd import cli
    import argparse
    ap = argparse.ArgumentParser()
    cp = cli.pairs_parser(ap.add_subparsers(dest="cmd"))
    args = cp.parse_args(["a.fa", "b.fa", "-k", "2", "--edit", "--rc", "--nearest"])
    assert (args.a, args.b, args.k, args.edit, args.rc, args.nearest) == ("a.fa", "b.fa", 2, True, True, True)
    assert cp.parse_args(["a.fa", "-k", "0"]).edit is False
    a = tmp_path / "a.txt"
    a.write_bytes(b"ACGT\nGGCC\n")
    shorter = tmp_path / "shorter.txt"
    shorter.write_bytes(b"ACG\nGGC\n")
    ragged = tmp_path / "ragged.txt"
    ragged.write_bytes(b"ACG\nGGCC\n")
    # without --edit one length for both sets, as before; with it a length per set -- but one inside each
    with pytest.raises(SystemExit):
        cli.main(["pairs", str(a), str(shorter), "-k", "1"])
    assert "sequence 0 has 3 bytes" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["pairs", str(a), str(ragged), "-k", "1", "--edit"])
    assert "sequence 1 has 4 bytes, the first of " + str(ragged) + " has 3" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["pairs", str(ragged), "-k", "1", "--edit"])
    assert "sequence 1 has 4 bytes" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["pairs", str(a), "-k", "255", "--edit"])
    assert "0 <= k <= 254" in capsys.readouterr().err


def test_cli_run_pairs_goes_through_the_edit_methods(sassy):
    """run_pairs on a stand-in searcher: --edit picks edit_pairs / edit_nearest, the rows are the Hamming verb's"""
    from sassy_amd import cli
    import io
    import types
    a = [("bc1", b"ACGT")]
    b = [("w1", b"CGTA"), ("w2", b"ACGT"), ("w3", b"TTTT"), ("w4", b"ACTG")]
    recs = np.zeros(len(eref.HAND_PAIRS), dtype=sassy.hamming_pair_dtype())
    for r, (i, j, s, c) in zip(recs, eref.HAND_PAIRS):
        r["a_idx"], r["b_idx"], r["strand"], r["cost"] = i, j, s, c
    calls = []

    class Stand:
        def edit_pairs(self, x, y, k):
            calls.append(("edit_pairs", x, y, k))
            return recs

        def edit_nearest(self, x, y, k):
            calls.append(("edit_nearest", x, y, k))
            return eref.expected_nearest("dna", x, y, k)

        def hamming_pairs(self, x, y, k):
            calls.append(("hamming_pairs", x, y, k))
            return recs[:0]

    out = io.StringIO()
    assert cli.run_pairs(types.SimpleNamespace(k=2, nearest=False, edit=True), Stand(), a, b, out) == 0
    assert out.getvalue() == cli.pairs_header() + "bc1\tw1\t+\t2\n" + "bc1\tw2\t+\t0\n" + "bc1\tw4\t+\t2\n"
    out = io.StringIO()
    assert cli.run_pairs(types.SimpleNamespace(k=2, nearest=True, edit=True), Stand(), a, b, out) == 0
    assert out.getvalue() == cli.pairs_header(nearest=True) + "bc1\tw2\t+\t0\t1\n"
    out = io.StringIO()
    assert cli.run_pairs(types.SimpleNamespace(k=2, nearest=False), Stand(), a, b, out) == 0  # (no --edit: the Hamming call)
    assert [c[0] for c in calls] == ["edit_pairs", "edit_nearest", "hamming_pairs"] and calls[0][1:] == ([b"ACGT"], [s for _, s in b], 2)
