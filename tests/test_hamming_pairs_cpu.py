"""CPU-only: the surface of the all-vs-all Hamming calls (sassy_hip_hamming_pairs, sassy_hip_hamming_nearest, the Python
methods, the `pairs` verb) -- what needs no device: the symbols, every refusal with its code and message before any device
work, the loud failure without a device, list and array inputs, the arithmetic of pairs_step.h driven by a stand-alone host
program under AddressSanitizer / UBSan, the helper on a hand-written case, the CLI's parser and row writers on canned
arrays."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import hamming_pairs_ref as pref  # noqa: E402

NAMES = ("sassy_hip_hamming_pairs", "sassy_hip_hamming_nearest")


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
    for name in NAMES + ("sassy_hip_hamming_pairs_free",):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(sassy.lib(), name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
    for name in NAMES:
        assert re.search(r"pub fn\s+" + name[len("sassy_hip_"):] + r"\s*\(", rust), name
    L = sassy.lib()
    assert L.sassy_hip_hamming_pairs.restype is not None and len(L.sassy_hip_hamming_pairs.argtypes) == 10
    assert L.sassy_hip_hamming_nearest.restype is not None and len(L.sassy_hip_hamming_nearest.argtypes) == 12
    assert "pairs_chunks" in [r[0] for r in sassy.option_table()]
    assert hasattr(sassy.Searcher, "hamming_pairs") and hasattr(sassy.Searcher, "hamming_nearest")
    dt = sassy.hamming_pair_dtype()
    assert dt.itemsize == 12 and dt.names == ("a_idx", "b_idx", "cost", "strand", "pad_")
    assert "sassy_hip_HammingPair" in hdr and "struct HammingPair" in rust
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"hamming_pairs.hip"' in build and '"pairs_step.h"' in build


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal of both entry points with its code and a message that names the reason, in a child that sees no device:
    a call that got as far as the device would say 'no usable HIP device' instead.  Then valid arguments: that message."""
    code = r'''
import ctypes as C, numpy as np, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
A = b"ACGTACGT" + b"TTTTACGT"
def call(which, s, a=A, n_a=2, b=None, n_b=0, m=8, k=1, flags=0, out=True, s_null=False):
    h = None if s_null else s._h
    if which == "pairs":
        o, n = C.c_void_p(), C.c_size_t()
        rc = L.sassy_hip_hamming_pairs(h, a, n_a, b, n_b, m, k, flags, C.byref(o) if out else None, C.byref(n) if out else None)
    else:
        cost = np.zeros(max(1, min(n_a, 16)), dtype=np.uint8)
        rc = L.sassy_hip_hamming_nearest(h, a, n_a, b, n_b, m, k, flags, cost.ctypes.data if out else None, None, None, None)
    return rc, L.sassy_hip_last_error().decode()
def refused(which, s, want, word, **kw):
    rc, msg = call(which, s, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (which, rc, msg, want, word)
dna = sassy_amd.Searcher("dna", rc=False)
for which in ("pairs", "nearest"):
    # the family's own checks
    refused(which, sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang")
    refused(which, sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match")
    refused(which, sassy_amd.Searcher("ascii", rc=True), EUNSUPPORTED, "reverse complement is not defined")
    refused(which, sassy_amd.Searcher("ascii_ci", rc=True), EUNSUPPORTED, "reverse complement is not defined")
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, "not valid IUPAC", a=b"ACGTACGT" + b"ACQTACGT")
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, "list a)", a=b"ACGTACGT" + b"ACQTACGT")  # (the message names the list)
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, "not valid IUPAC", b=b"ACGTAC1T", n_b=1)  # (the second list too)
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, "list b)", b=b"ACGTAC1T", n_b=1)
    # ... the family's Ascii limit of 64 distinct bytes per sequence included, "pattern N" counting inside the list named
    for alphabet in ("ascii", "ascii_ci"):
        wide = bytes(range(128, 193))
        refused(which, sassy_amd.Searcher(alphabet, rc=False), EUNSUPPORTED, "distinct bytes (pattern 1 has 65)", a=b"x" * 65 + wide, m=65)
        refused(which, sassy_amd.Searcher(alphabet, rc=False), EUNSUPPORTED, "list b)", a=b"x" * 130, m=65, b=b"y" * 65 + wide, n_b=2)
    # there is no text span for max_n_frac
    refused(which, sassy_amd.Searcher("dna", rc=False).with_max_n_frac(0.2), EUNSUPPORTED, "max_n_frac")
    # the shape
    refused(which, dna, EINVAL, "m must be at least 1", m=0)
    refused(which, dna, EINVAL, "m must be <= 128", a=b"A" * 258, m=129)
    refused(which, dna, EINVAL, "k must be <= 254", k=255)
    refused(which, dna, EINVAL, "k must be <= 254", k=0x80000000)
    refused(which, dna, EINVAL, "at least one sequence", n_a=0)
    refused(which, dna, EINVAL, "n_b is 0", b=A, n_b=0)
    refused(which, dna, EINVAL, "b is NULL", b=None, n_b=2)
    for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.ALL_MINIMA, sassy_amd.TEXT_ON_DEVICE, sassy_amd.TEXT_UNCHANGED, sassy_amd.LINE_SPANS, 1 << 20):
        refused(which, dna, EINVAL, "takes no flags", flags=flags)
    refused(which, dna, EUNSUPPORTED, "2^31 - 1", n_a=1 << 31)
    refused(which, dna, EUNSUPPORTED, "2^31 - 1", b=A, n_b=1 << 31)
    refused(which, dna, EINVAL, "must not be null", out=False)
    refused(which, dna, EINVAL, "must not be null", a=None)
    refused(which, dna, EINVAL, "must not be null", s_null=True)
    # valid arguments get as far as the device: every alphabet, both modes, the limits themselves
    for s, kw in ((dna, {}), (dna, dict(b=A, n_b=2)), (sassy_amd.Searcher("dna", rc=True), dict(k=254)),
                  (sassy_amd.Searcher("iupac", rc=True), dict(a=b"ACGTNNRY" * 2)), (sassy_amd.Searcher("ascii", rc=False), {}),
                  (sassy_amd.Searcher("ascii_ci", rc=False), dict(a=b"x" * 256, m=128)), (dna, dict(a=b"AC", m=1))):
        rc, msg = call(which, s, **kw)
        assert rc == ENODEVICE and "no usable HIP device" in msg, (which, rc, msg)
# the Python methods: refusals of their own, then the same loud failure
for method in ("hamming_pairs", "hamming_nearest"):
    f = getattr(dna, method)
    for args, word in ((([b"ACGT", b"ACG"],), "sequence 1 has 3 bytes"), (([b"ACGT"], [b"ACGTA"]), "b has 5 bytes"),
                       (([b"ACGT", sassy_amd.parse_classes(b"a[bc]")],), "ClassPattern"), ((sassy_amd.parse_classes(b"a[bc]"),), "ClassPattern"),
                       ((np.zeros((2, 4), dtype=np.int32),), "uint8 array"), ((np.zeros((4, 4), dtype=np.uint8)[:, ::2],), "C-contiguous"),
                       (([b"ACGT"], None, 300), "k must be <= 254"), (([],), "needs at least one sequence"),
                       (([b"ACGT"], []), "b holds no sequence"), ((np.zeros((0, 4), dtype=np.uint8),), "needs at least one sequence"), (([b"ACGT", b"AAAA"],), "no usable HIP device"),
                       ((np.frombuffer(b"ACGTAAAA", dtype=np.uint8).reshape(2, 4), [b"ACGT"], 1), "no usable HIP device")):
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


def test_refusals_are_the_familys_function():
    """No copy of the family's checks: the new unit calls hamming_refusals once, for both entry points and both lists, and
    reads neither the environment nor holds the strings hamming.hip is pinned to hold once."""
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "hamming_pairs.hip")).read()
    assert src.count("hamming_refusals(") == 1 and src.count("pairs_refusals(") == 3 and src.count("family(") == 2  # (once per list)
    body = src[src.index("int pairs_refusals("):]
    body = body[:body.index("\n}\n")]
    assert "hamming_refusals(" in body
    for entry in ("int sassy_hip_hamming_pairs(", "int sassy_hip_hamming_nearest("):
        fn = src[src.index(entry):]
        assert fn.index("pairs_refusals(") < fn.index("hamming_call(")  # (hamming_call: the device)
    assert "only_best_match" not in src and "SASSY_NO_TICKETS" not in src and "getenv" not in src


def test_list_and_array_inputs_marshal_to_the_same_bytes(sassy):
    seqs = [b"ACGTAC", b"TTTTTT", b"acgtnn", bytes(range(6))]
    from_list = sassy.pairs_sequences(seqs)
    arr = np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(4, 6).copy()
    from_array = sassy.pairs_sequences(arr)
    assert from_array is arr  # (no copy, per entry or otherwise)
    assert from_list.shape == (4, 6) and from_list.dtype == np.uint8 and from_list.flags["C_CONTIGUOUS"]
    assert from_list.tobytes() == from_array.tobytes() == b"".join(seqs)
    assert sassy.pairs_sequences([bytearray(b"AC"), memoryview(b"GT")]).tobytes() == b"ACGT"
    with pytest.raises(sassy.SassyHipError, match="sequence 2 has 5 bytes, sequence 0 has 4"):
        sassy.pairs_sequences([b"ACGT", b"ACGT", b"ACGTA", b"AC"])
    with pytest.raises(sassy.SassyHipError, match="not one sequence"):
        sassy.pairs_sequences(b"ACGT")


def test_pairs_arithmetic_against_brute_force_under_sanitizers(tmp_path):
    """tests/c/pairs_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: encoding and per-word distance against a byte-wise count for every profile and
    m in {1, 31, 32, 33, 63, 64, 65, 96, 127, 128}, the combine rule against a sequential walk, the plan's coverage."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pairs_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "pairs_step_driver.cc")])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
        assert int(fields["costs"]) == 4 * 10 * 60 and int(fields["combines"]) == 2000
        assert int(fields["plans"]) == (8 * 8 + 2 * 8) * 5 and int(fields["cells"]) > 1000


def test_step_header_stays_free_of_hip():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "pairs_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "getenv" not in src
    assert "__builtin_amdgcn" not in src and "__HIP_DEVICE_COMPILE__" not in src
    for name in ("pairs_encode", "pairs_mismatch_word", "pairs_cost", "pairs_combine", "pairs_plan", "pairs_tile_first", "pairs_visits"):
        assert re.search(r"\b" + name + r"\s*[<(]", src), name
    # the kernels and the host share it
    unit = open(os.path.join(ROOT, "sassy_amd", "csrc", "hamming_pairs.hip")).read()
    for name in ("pairs_encode(", "pairs_cost<", "pairs_combine(", "pairs_plan(", "pairs_tile_first(", "pairs_visits("):
        assert name in unit, name


# ---------------------------------------------------------------- the helper, on a case written out by hand
def test_helper_on_a_hand_written_case():
    t = pref.as_tuples
    assert t(pref.expected_pairs("dna", pref.HAND_SELF, None, pref.HAND_K, rc=True)) == pref.HAND_SELF_PAIRS_RC
    assert t(pref.expected_pairs("dna", pref.HAND_SELF, None, pref.HAND_K, rc=False)) == pref.HAND_SELF_PAIRS_FWD
    assert t(pref.expected_pairs("dna", pref.HAND_A, pref.HAND_B, pref.HAND_K)) == pref.HAND_TWO_PAIRS
    rows = lambda cols: [tuple(int(c[i]) for c in cols) for i in range(len(cols[0]))]
    assert rows(pref.expected_nearest("dna", pref.HAND_SELF, None, pref.HAND_K, rc=True)) == pref.HAND_SELF_NEAREST_RC
    assert rows(pref.expected_nearest("dna", pref.HAND_SELF, None, pref.HAND_K, rc=False)) == pref.HAND_SELF_NEAREST_FWD
    assert rows(pref.expected_nearest("dna", pref.HAND_A, pref.HAND_B, pref.HAND_K)) == pref.HAND_TWO_NEAREST
    # two-set mode of a list against itself is the square: the triangle's strand-0 pairs both ways round, and the diagonal
    square = t(pref.expected_pairs("dna", pref.HAND_SELF, pref.HAND_SELF, pref.HAND_K))
    assert square == [(0, 0, 0, 0), (0, 1, 0, 1), (1, 0, 0, 1), (1, 1, 0, 0), (2, 2, 0, 0), (3, 3, 0, 0)]
    # the relation is the family's: Dna compares (c >> 1) & 3 -- lower case matches upper case, and so do bytes that share the
    # code; Iupac N meets everything, disjoint sets cost one
    assert t(pref.expected_pairs("dna", [b"acgt"], [b"ACGT", b"ACGU"], 0)) == [(0, 0, 0, 0), (0, 1, 0, 0)]
    assert t(pref.expected_pairs("iupac", [b"NNNN", b"ACGT"], [b"ACGT", b"RYKM"], 1)) == [(0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 0, 1)]
    assert t(pref.expected_pairs("ascii_ci", [b"abc"], [b"ABC", b"AB@"], 0)) == [(0, 0, 0, 0)]
    assert t(pref.expected_pairs("ascii", [b"abc"], [b"ABC", b"abc"], 0)) == [(0, 1, 0, 0)]


# ---------------------------------------------------------------- CLI
def test_cli_pairs_parser(sassy, capsys, tmp_path):
    from sassy_amd import cli
    a = tmp_path / "a.txt"
    a.write_bytes(b"ACGT\nGGCC\n")
    with pytest.raises(SystemExit):
        cli.main(["pairs", str(a)])  # no k
    with pytest.raises(SystemExit):
        cli.main(["pairs", str(a), "-k", "255"])
    assert "0 <= k <= 254" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["pairs", str(a), "-k", "1", "--rc", "-a", "ascii"])
    assert "no reverse complement" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["pairs", str(a), "-k", "1", "-a", "protein"])
    ragged = tmp_path / "ragged.txt"
    ragged.write_bytes(b"ACGT\nGGC\n")
    with pytest.raises(SystemExit):
        cli.main(["pairs", str(ragged), "-k", "1"])  # (refused by the front end: no device is asked for)
    assert "sequence 1 has 3 bytes" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["pairs", str(a), str(ragged), "-k", "1"])
    assert "sequence 1 has 3 bytes" in capsys.readouterr().err
    import argparse
    ap = argparse.ArgumentParser()
    cp = cli.pairs_parser(ap.add_subparsers(dest="cmd"))
    args = cp.parse_args([str(a), "b.fa", "-k", "2", "--rc", "--nearest", "-a", "IUPAC"])
    assert (args.a, args.b, args.k, args.rc, args.nearest, args.alphabet) == (str(a), "b.fa", 2, True, True, "iupac")
    args = cp.parse_args([str(a), "-k", "0"])
    assert (args.b, args.rc, args.nearest, args.alphabet) == (None, False, False, "dna")


def test_cli_pairs_row_writers_on_canned_arrays(sassy):
    from sassy_amd import cli
    a = [("bc1", b"ACGT"), ("bc2", b"ACGA"), ("bc3", b"TTTT"), ("bc4", b"AAAT")]
    b = [("w1", b"ACGA"), ("w2", b"ACGT")]
    assert cli.pairs_header() == "a_id\tb_id\tstrand\tcost\n"
    assert cli.pairs_header(nearest=True) == "a_id\tb_id\tstrand\tcost\tties\n"
    recs = np.zeros(len(pref.HAND_SELF_PAIRS_RC), dtype=sassy.hamming_pair_dtype())
    for r, (i, j, s, c) in zip(recs, pref.HAND_SELF_PAIRS_RC):
        r["a_idx"], r["b_idx"], r["strand"], r["cost"] = i, j, s, c
    assert cli.pairs_rows(a, a, recs) == ["bc1\tbc1\t-\t0\n", "bc1\tbc2\t+\t1\n", "bc1\tbc2\t-\t1\n", "bc3\tbc4\t-\t1\n"]
    assert cli.pairs_rows(a, b, recs[:0]) == []
    cost = np.array([0, 255], dtype=np.uint8)
    index = np.array([1, 0xFFFFFFFF], dtype=np.uint32)
    strand = np.array([1, 0], dtype=np.uint8)
    ties = np.array([3, 0], dtype=np.uint32)
    assert cli.nearest_rows(a[:2], b, cost, index, strand, ties) == ["bc1\tw2\t-\t0\t3\n", "bc2\t*\t*\t-1\t0\n"]
