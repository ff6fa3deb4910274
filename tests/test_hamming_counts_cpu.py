"""CPU-only: the counting Hamming calls' surface (sassy_hip_hamming_counts, sassy_hip_hamming_counts_many, the Python methods,
the `count` verb) -- what needs no device: the symbols, every refusal with its code and message before any device work, the
loud failure without a device, the arithmetic hamming_step.h adds driven by a stand-alone host program under AddressSanitizer
/ UBSan, the helper on a hand-written case, the CLI's parser and row writers on canned tables."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import hamming_counts_ref as cref  # noqa: E402
import hamming_many_ref as mref  # noqa: E402

NAMES = ("sassy_hip_hamming_counts", "sassy_hip_hamming_counts_many")


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
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(sassy.lib(), name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
        assert re.search(r"pub fn\s+" + name[len("sassy_hip_"):] + r"\s*\(", rust), name
    L = sassy.lib()
    assert L.sassy_hip_hamming_counts.restype is not None and len(L.sassy_hip_hamming_counts.argtypes) == 9
    assert L.sassy_hip_hamming_counts_many.restype is not None and len(L.sassy_hip_hamming_counts_many.argtypes) == 10
    assert "hamming_count_copies" in [r[0] for r in sassy.option_table()]
    assert hasattr(sassy.Searcher, "hamming_counts") and hasattr(sassy.Searcher, "hamming_counts_many")


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal of both entry points with its code and a message that names the reason, in a child that sees no device:
    a call that got as far as the device would say 'no usable HIP device' instead.  Then valid arguments: that message.
    n_texts == 0 is a zero table without a device."""
    code = r'''
import ctypes as C, numpy as np, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
def call(which, s, pats, texts=(b"ACGTACGTACGTACGT", b"", b"ACG"), k=1, flags=0, out=True):
    pp = (C.c_char_p * max(1, len(pats)))(*pats)
    pl = (C.c_size_t * max(1, len(pats)))(*[len(p) for p in pats])
    table = np.full(max(1, len(pats)) * 2 * (min(k, 254) + 1), 7, dtype=np.uint64)
    addr = table.ctypes.data if out else None
    if which == "many":
        keep = [C.create_string_buffer(t, max(1, len(t))) for t in texts]
        tp = (C.c_void_p * max(1, len(texts)))(*[C.addressof(b) for b in keep])
        tl = (C.c_size_t * max(1, len(texts)))(*[len(t) for t in texts])
        rc = L.sassy_hip_hamming_counts_many(s._h, pp, pl, len(pats), tp, tl, len(texts), k, flags, addr)
    else:
        rc = L.sassy_hip_hamming_counts(s._h, pp, pl, len(pats), texts[0], len(texts[0]), k, flags, addr)
    return rc, L.sassy_hip_last_error().decode(), table
def refused(which, s, want, word, *a, **kw):
    rc, msg, _ = call(which, s, *a, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (which, rc, msg, want, word)
dna = sassy_amd.Searcher("dna", rc=False)
for which in ("one", "many"):
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
    refused(which, dna, EINVAL, "k must be <= 254", [b"ACGT"], k=255)
    refused(which, dna, EINVAL, "k must be <= 254", [b"ACGT"], k=0x80000000)
    refused(which, dna, EINVAL, "must not be null", [b"ACGT"], out=False)
    for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.ALL_MINIMA, sassy_amd.LINE_SPANS, 1 << 20):
        refused(which, dna, EINVAL, "hamming_counts_many takes no flags" if which == "many" else "hamming_counts takes", [b"ACGT"], flags=flags)
for flags in (sassy_amd.TEXT_ON_DEVICE, sassy_amd.TEXT_UNCHANGED):
    refused("many", dna, EINVAL, "host texts only", [b"ACGT"], flags=flags)
# a table of more than 2^32 - 1 bins: 2^32 / 510 patterns at k = 254, all one buffer (no table that large is touched)
n = (1 << 32) // 510 + 1
one = C.create_string_buffer(b"ACGT")
pp = np.full(n, C.addressof(one), dtype=np.uint64); pl = np.full(n, 4, dtype=np.uint64); out = np.zeros(1, dtype=np.uint64)
ptr = lambda a: C.cast(a.ctypes.data, C.c_void_p)
L.sassy_hip_hamming_counts.argtypes = [C.c_void_p] * 3 + list(L.sassy_hip_hamming_counts.argtypes[3:])
L.sassy_hip_hamming_counts_many.argtypes = [C.c_void_p] * 3 + list(L.sassy_hip_hamming_counts_many.argtypes[3:])
assert L.sassy_hip_hamming_counts(dna._h, ptr(pp), ptr(pl), n, b"ACGT", 4, 254, 0, ptr(out)) == EUNSUPPORTED
assert "2^32 - 1 bins" in L.sassy_hip_last_error().decode()
tp = (C.c_void_p * 1)(C.addressof(one)); tl = (C.c_size_t * 1)(4)
assert L.sassy_hip_hamming_counts_many(dna._h, ptr(pp), ptr(pl), n, tp, tl, 1, 254, 0, ptr(out)) == EUNSUPPORTED
assert "2^32 - 1 bins" in L.sassy_hip_last_error().decode() and out[0] == 0
# null pointers
assert L.sassy_hip_hamming_counts(None, None, None, 0, None, 0, 0, 0, None) == EINVAL
assert L.sassy_hip_hamming_counts_many(None, None, None, 0, None, None, 0, 0, 0, None) == EINVAL
assert L.sassy_hip_hamming_counts_many(dna._h, ptr(pp), ptr(pl), 1, None, None, 2, 1, 0, ptr(out)) == EINVAL
assert "must not be null" in L.sassy_hip_last_error().decode()
# n_texts == 0: a zero table, 0 -- and no device is asked for
rc, msg, table = call("many", dna, [b"ACGT", b"AC"], texts=(), k=3)
assert rc == 0 and not table.any(), (rc, msg)
assert dna.hamming_counts_many([b"ACGT"], [], 2).tolist() == [[[0, 0, 0], [0, 0, 0]]]
# valid arguments get as far as the device
for which, s, pats, k in (("many", sassy_amd.Searcher("ascii_ci", rc=False), [bytes(range(65, 91)) + bytes(range(97, 123))], 1),
                          ("one", dna, [b"A" * 1024], 254), ("many", dna, [b"A" * 1024], 254),
                          ("one", sassy_amd.Searcher("dna", rc=True), [b"ACGT"], 0),
                          ("one", sassy_amd.Searcher("ascii", rc=False), [bytes(range(64)), bytes(range(64, 128))], 0)):
    rc, msg, _ = call(which, s, pats, k=k)
    assert rc == ENODEVICE and "no usable HIP device" in msg, (which, rc, msg)
for method, text in (("hamming_counts", b"abc"), ("hamming_counts_many", [b"abc"])):
    for pats in (sassy_amd.parse_classes(b"a[bc]"), [b"ACGT", sassy_amd.parse_classes(b"a[bc]")]):
        try:
            getattr(dna, method)(pats, text, 0)
        except sassy_amd.SassyHipError as e:
            assert "ClassPattern" in str(e), e
        else:
            raise SystemExit(3)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_refusals_are_the_familys_function():
    """No copy of the checks: both counting entry points go through one function that calls hamming_refusals once, which ends
    in the open-tickets check."""
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "hamming.hip")).read()
    body = src[src.index("int hamming_count_call("):]
    body = body[:body.index("\n}\n")]
    assert body.count("hamming_refusals(") == 1 and body.index("hamming_refusals(") < body.index("hamming_call(")  # (hamming_call: the device)
    assert src.count("int hamming_count_call(") == 1 and src.count("return hamming_count_call(s, patterns,") == 2
    assert src.count("only_best_match is not supported") == 1 and src.count("SASSY_NO_TICKETS") == 1


def test_no_device_fails_loudly(sassy):
    code = (
        "import sassy_amd\n"
        "assert sassy_amd.device_count() == 0\n"
        "for alphabet, rc in (('dna', True), ('iupac', False), ('ascii', False), ('ascii_ci', False)):\n"
        "    s = sassy_amd.Searcher(alphabet, rc=rc)\n"
        "    for pats in (b'ACGT', [b'ACGT', b'AC']):\n"
        "        for call in (lambda: s.hamming_counts(pats, b'ACGTACGTACGT', 1), lambda: s.hamming_counts_many(pats, [b'ACGTACGT', b''], 1)):\n"
        "            try:\n"
        "                call()\n"
        "            except sassy_amd.SassyHipError as e:\n"
        "                assert 'no usable HIP device' in str(e), e\n"
        "            else:\n"
        "                raise AssertionError('no SassyHipError')\n"
        "print('ok')\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_counting_arithmetic_against_brute_force_under_sanitizers(tmp_path):
    """tests/c/hamming_counts_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: eq(c) for P in {2, 4, 8, 11} and every c < 2^P with `over` on some, none and all starts,
    the partition of le(k), the min / max cost helpers on the narrowing driver's masks, the fold's popcounts."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hamming_counts_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "hamming_counts_step_driver.cc")])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
        assert int(fields["eqs"]) == int(fields["partitions"]) == 200 * 4 + 200 * 16 + 100 * 256 + 20 * 2048
        assert int(fields["bounds"]) == 4 * 400 * (7 + 6) and int(fields["folds"]) > 4 * 400 * 3


def test_step_header_stays_free_of_hip():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "hamming_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src
    outside = re.sub(r"#if defined\(__HIP_DEVICE_COMPILE__\).*?#else", "", src, flags=re.S)
    assert "__builtin_amdgcn" not in outside
    for name in ("eq", "le", "ham_min_cost", "ham_max_cost", "ham_count"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    assert "exact for every v <= k" in src  # the comment the contract of eq rests on


# ---------------------------------------------------------------- the helper, on a case written out by hand
def test_helper_on_a_hand_written_case():
    pats, texts, k = cref.HAND_PATTERNS, cref.HAND_TEXTS, cref.HAND_K
    for text, want in zip(texts, cref.HAND_PER_TEXT):
        got = cref.expected_counts("dna", pats, text, k, rc=True)
        assert got.dtype == np.uint64 and got.shape == (2, 2, 2) and got.tolist() == want, text
    assert cref.expected_counts("dna", pats, texts, k, rc=True).tolist() == cref.HAND_TOTAL
    # without rc the '-' rows are zero and the '+' rows stay
    fwd = cref.expected_counts("dna", pats, texts, k, rc=False)
    assert fwd[:, 0].tolist() == [r[0] for r in cref.HAND_TOTAL] and not fwd[:, 1].any()
    # the table is the count of the batch helper's records
    rows = mref.expected_many("dna", pats, texts, k, rc=True, without_trace=True)
    again = np.zeros((2, 2, 2), dtype=np.uint64)
    for _, x in rows:
        again[x.pattern_idx, 0 if x.strand == "+" else 1, x.cost] += 1
    assert again.tolist() == cref.HAND_TOTAL
    # a larger k only adds columns; a pattern longer than the text has zero rows; the N rule drops spans
    wide = cref.expected_counts("dna", pats, texts, 3, rc=True)
    assert wide[:, :, :2].tolist() == cref.HAND_TOTAL and wide.shape == (2, 2, 4) and not wide[1, :, 3].any()
    assert not cref.expected_counts("dna", [b"ACGTACGTACGT"], b"ACGT", 2).any()
    # Iupac: the text's N matches every base, so ACNT is a hit of cost 0 -- until the N rule drops its span
    assert cref.expected_counts("iupac", [b"ACGT"], b"ACNTACGT", 1).tolist() == [[[2, 0], [0, 0]]]
    assert cref.expected_counts("iupac", [b"ACGT"], b"ACNTACGT", 1, max_n_frac=0.0).tolist() == [[[1, 0], [0, 0]]]


# ---------------------------------------------------------------- CLI
def test_cli_count_parser(sassy, capsys, tmp_path):
    from sassy_amd import cli
    pats = tmp_path / "pats.txt"
    pats.write_bytes(b"ACGT\n\nGGCC\r\n")
    assert cli.load_count_patterns(str(pats)) == [("1", b"ACGT"), ("2", b"GGCC")]
    fa = tmp_path / "pats.fa"
    fa.write_bytes(b">g1 first\nACGT\n>g2\nGG\nCC\n")
    assert [(i.split()[0], p) for i, p in cli.load_count_patterns(str(fa))] == [("g1", b"ACGT"), ("g2", b"GGCC")]
    with pytest.raises(SystemExit):
        cli.main(["count", str(pats), "-k", "1"])  # no FASTX
    with pytest.raises(SystemExit):
        cli.main(["count", str(pats), "nofile.fa"])  # no k
    with pytest.raises(SystemExit):
        cli.main(["count", str(pats), "nofile.fa", "-k", "255"])
    assert "0 <= k <= 254" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["count", str(pats), "nofile.fa", "-k", "1", "--rc", "--alphabet", "ascii"])
    assert "no reverse complement" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["count", str(pats), "nofile.fa", "-k", "1", "--overhang", "0.5"])


def test_cli_count_row_writers_on_canned_tables():
    from sassy_amd import cli
    patterns = [("g1", b"ACGT"), ("g2", b"GG")]
    table = np.array(cref.HAND_TOTAL, dtype=np.uint64)
    assert cli.count_header(1) == "pat_id\tstrand\tn_0\tn_1\n"
    assert cli.count_header(3, per_record=True) == "text_id\tpat_id\tstrand\tn_0\tn_1\tn_2\tn_3\n"
    assert cli.count_rows(patterns, table, rc=True) == ["g1\t+\t1\t2\n", "g1\t-\t1\t2\n", "g2\t+\t1\t6\n", "g2\t-\t1\t4\n"]
    assert cli.count_rows(patterns, table, rc=False) == ["g1\t+\t1\t2\n", "g2\t+\t1\t6\n"]
    assert cli.count_rows(patterns, table, rc=True, text_id="chr1") == ["chr1\tg1\t+\t1\t2\n", "chr1\tg1\t-\t1\t2\n", "chr1\tg2\t+\t1\t6\n",
                                                                      "chr1\tg2\t-\t1\t4\n"]
    big = np.array([[[2 ** 40 + 1, 0], [0, 0]]], dtype=np.uint64)  # counters are 64-bit: written as integers
    assert cli.count_rows([("p", b"A")], big, rc=False) == [f"p\t+\t{2 ** 40 + 1}\t0\n"]
