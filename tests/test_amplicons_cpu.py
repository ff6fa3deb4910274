"""CPU-only: the amplicon call's surface (sassy_hip_hamming_amplicons, sassy_hip_amplicons_free, Searcher.hamming_amplicons,
the `amplicon` verb) -- what needs no device: the symbols, every refusal with its code and message before any device work,
the loud failure without a device, the join's arithmetic (amplicon_step.h) driven by a stand-alone host program under
AddressSanitizer / UBSan, the helper on a hand-written case, the CLI's parser, primer-file reader and row writer on canned
records."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import amplicon_ref as aref  # noqa: E402

NAMES = ("sassy_hip_hamming_amplicons", "sassy_hip_amplicons_free")


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
    assert "SASSY_HIP_AMPLICON_MAX_LEN (1u << 24)" in hdr and "} sassy_hip_Amplicon;" in hdr
    L = sassy.lib()
    assert L.sassy_hip_hamming_amplicons.restype is not None and len(L.sassy_hip_hamming_amplicons.argtypes) == 14
    assert hasattr(sassy.Searcher, "hamming_amplicons")
    dt = sassy.amplicon_dtype()
    assert dt.itemsize == 24 and dt == aref.DTYPE
    assert '"amplicons.hip"' in open(os.path.join(ROOT, "sassy_amd", "build.py")).read()


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal with its code and a message that names the reason, in a child that sees no device: a call that got as
    far as the device would say 'no usable HIP device' instead.  Then valid arguments: that message."""
    code = r'''
import ctypes as C, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
def call(s, pairs, text=b"ACGTACGTACGTACGTACGT", k=1, min_len=4, max_len=12, flags=0, out=True):
    n = len(pairs)
    fp = (C.c_char_p * max(1, n))(*[f for f, _ in pairs]); fl = (C.c_size_t * max(1, n))(*[len(f) for f, _ in pairs])
    rp = (C.c_char_p * max(1, n))(*[r for _, r in pairs]); rl = (C.c_size_t * max(1, n))(*[len(r) for _, r in pairs])
    res, cnt = C.c_void_p(7), C.c_size_t(7)
    rc = L.sassy_hip_hamming_amplicons(s._h, fp, fl, rp, rl, n, text, len(text), k, min_len, max_len, flags, C.byref(res) if out else None,
                                       C.byref(cnt))
    return rc, L.sassy_hip_last_error().decode(), res.value, cnt.value
def refused(s, want, word, *a, **kw):
    rc, msg, res, cnt = call(s, *a, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (rc, msg, want, word)
    if kw.get("out", True):
        assert res is None and cnt == 0, (res, cnt)  # nothing comes back
dna = sassy_amd.Searcher("dna", rc=True)
ok = [(b"ACGT", b"ACGT")]
# what the whole Hamming family refuses, for any of the 2 n_pairs primers
refused(sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang", ok)
refused(sassy_amd.Searcher("dna", rc=True).only_best_match(), EUNSUPPORTED, "only_best_match", ok)
refused(dna, EINVAL, "at least one pattern", [])
refused(dna, EINVAL, "empty pattern (pattern 1)", [(b"ACGT", b"")])
refused(dna, EINVAL, "empty pattern (pattern 2)", [(b"ACGT", b"ACGT"), (b"", b"ACGT")])
refused(sassy_amd.Searcher("iupac", rc=True), EINVAL, "not valid IUPAC", [(b"ACGT", b"ACGT"), (b"ACGT", b"ACQT")])
refused(dna, EUNSUPPORTED, "at most 1024 rows (pattern 3", [(b"ACGT", b"ACGT"), (b"ACGT", b"A" * 1025)], max_len=2000)
# the amplicon call's own
for alphabet in ("ascii", "ascii_ci"):
    for rc in (False, True):
        refused(sassy_amd.Searcher(alphabet, rc=rc), EUNSUPPORTED, "reverse complement is not defined", ok)
refused(dna, EINVAL, "k must be <= 254", ok, k=255)
refused(dna, EINVAL, "k must be <= 254", ok, k=0x80000000)
refused(dna, EINVAL, "min_len must be at least 1", ok, min_len=0)
refused(dna, EINVAL, "larger than max_len", ok, min_len=13, max_len=12)
refused(dna, EINVAL, "SASSY_HIP_AMPLICON_MAX_LEN", ok, max_len=(1 << 24) + 1)
for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.ALL_MINIMA, sassy_amd.LINE_SPANS, 1 << 20):
    refused(dna, EINVAL, "hamming_amplicons takes SASSY_HIP_TEXT_ON_DEVICE", ok, flags=flags)
refused(dna, EINVAL, "must not be null", ok, out=False)
assert L.sassy_hip_hamming_amplicons(None, None, None, None, None, 0, None, 0, 0, 1, 1, 0, None, None) == EINVAL
L.sassy_hip_amplicons_free(None)
# valid arguments get as far as the device
for s, pairs, kw in ((dna, ok, {}), (sassy_amd.Searcher("iupac", rc=False), [(b"ACRYN", b"NNAC")], {}), (dna, ok, dict(max_len=1 << 24)),
                     (dna, [(b"A" * 1024, b"C" * 1024)], dict(k=254, min_len=1, max_len=1 << 24)),
                     (dna, [(b"A" * 40, b"ACGT")], {}), (dna, ok, dict(flags=sassy_amd.TEXT_UNCHANGED))):
    rc, msg, _, _ = call(s, pairs, **kw)
    assert rc == ENODEVICE and "no usable HIP device" in msg, (rc, msg)
try:
    dna.hamming_amplicons(ok, b"ACGTACGTACGT", 1, 4, 10)
except sassy_amd.SassyHipError as e:
    assert "no usable HIP device" in str(e), e
else:
    raise SystemExit(3)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_refusals_and_scan_are_the_familys_functions():
    """No copy of the checks and none of the scan: the entry point hands all primers to the family's refusals once, before the
    device (hamming_call), and the driver scans through the one range walker -- and so through ham_scan_range -- as the record
    driver of hamming.hip does; amplicons.hip has no scan kernel."""
    amp = open(os.path.join(ROOT, "sassy_amd", "csrc", "amplicons.hip")).read()
    ham = open(os.path.join(ROOT, "sassy_amd", "csrc", "hamming.hip")).read()
    shared = open(os.path.join(ROOT, "sassy_amd", "csrc", "host_internal.h")).read()
    assert amp.count("hamming_refusals(") == 1 and amp.index("hamming_refusals(") < amp.index("hamming_call(")
    assert "ensure_device" not in amp and "ensure_device()" in shared[shared.index("int hamming_call("):shared.index("int ham_one_text(")]
    assert "SASSY_NO_TICKETS" not in amp and "only_best_match" not in amp
    assert ham.count("\nint hamming_refusals(") == 1 and "hamming_family_refusals" not in amp + ham + shared
    assert amp.count("ham_walk_ranges(S, J, P") == 1 and ham.count("ham_walk_ranges(S, J, P") == 1
    assert shared.count("ham_scan_range(S, J, P") == 1 and "ham_scan_range(" not in amp
    assert "ham_scan_kernel" not in amp and "launch_scan" not in amp
    assert "__global__" in amp and "amp_count_kernel" in amp and "amp_emit_kernel" in amp
    assert "asm" not in re.sub(r"//.*", "", amp)


def test_join_arithmetic_against_brute_force_under_sanitizers(tmp_path):
    """tests/c/amplicon_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: the partner window against the definition, the lower bound inside a run, counts and the
    j-th start over runs with missing blocks for windows ending on bit 0, bit 63 and next to them, empty and one-start
    windows, j first, last and out of range, and the ownership of every start by exactly one of the overlapping ranges."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "amplicon_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "amplicon_step_driver.cc")])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
        assert int(fields["windows"]) == 402 and int(fields["owners"]) == 200
        assert int(fields["bounds"]) > 500 and int(fields["counts"]) > 10000 and int(fields["selects"]) > 5 * int(fields["counts"])


def test_step_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "amplicon_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "__builtin_amdgcn" not in src
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>"]
    for name in ("amp_window", "amp_lower_bound", "amp_count", "amp_select", "amp_owns", "amp_next_from", "amp_min_span"):
        assert re.search(r"\b" + name + r"\s*\(", src), name


# ---------------------------------------------------------------- the helper, on a case written out by hand
def test_helper_on_a_hand_written_case():
    plus = aref.expected("dna", [aref.HAND_PAIR], aref.HAND_TEXT, 0, 4, 80, rc=False)
    assert plus.dtype == aref.DTYPE and len(plus) == aref.HAND_COUNT == 2701
    assert not plus["strand"].any() and not plus["pair_idx"].any() and not plus["fwd_cost"].any() and not plus["rev_cost"].any()
    assert (int(plus[0]["start"]), int(plus[0]["end"])) == aref.HAND_FIRST == (74, 154)
    assert (int(plus[-1]["start"]), int(plus[-1]["end"])) == aref.HAND_LAST == (146, 226)
    length = plus["end"].astype(np.int64) - plus["start"].astype(np.int64)
    assert length.min() == 8 and length.max() == 80  # d = p - s in [4, 76], L = d + 4
    d, n = np.unique(length - 4, return_counts=True)
    assert d.tolist() == list(range(4, 77)) and n.tolist() == [x - 3 for x in range(4, 77)]
    both = aref.expected("dna", [aref.HAND_PAIR], aref.HAND_TEXT, 0, 4, 80, rc=True)
    assert len(both) == 2 * 2701 and aref.same(both[:2701], plus)
    minus = both[2701:].copy()
    assert minus["strand"].all()
    minus["strand"] = 0
    assert aref.same(minus, plus)  # F == R: both strands on every span
    # order: (pair_idx, strand, start, end)
    key = list(zip(both["pair_idx"].tolist(), both["strand"].tolist(), both["start"].tolist(), both["end"].tolist()))
    assert key == sorted(key)
    # costs name the primer, not the side: F = ACGT at 0 with one mismatch, R = TTGG whose reverse complement CCAA ends at 12
    text = b"ACCTAAAACCAA" + b"TTGGAAAAAGGT"
    r = aref.expected("dna", [(b"ACGT", b"TTGG")], text, 1, 12, 12, rc=True)
    assert [tuple(int(v) for v in x) for x in r.tolist()] == [(0, 12, 0, 0, 1, 0, 0), (12, 24, 0, 1, 1, 0, 0)]
    assert len(aref.expected("dna", [(b"ACGT", b"TTGG")], text, 0, 12, 12, rc=True)) == 0
    # L >= max(a, b): the right site may lie inside the left one, but not end in front of its end
    inside = aref.expected("dna", [(b"AAAAAA", b"TT")], b"CCAAAAAACC", 0, 1, 10, rc=False)
    assert [(int(x["start"]), int(x["end"])) for x in inside] == [(2, 8)]  # of the five AA only the one that ends at 8
    assert len(aref.expected("dna", [(b"AAAAAA", b"TT")], b"CCAAAAAACC", 0, 1, 5, rc=False)) == 0
    assert len(aref.expected("dna", [(b"AAAT", b"AT")], b"CCAAATCC", 0, 1, 10, rc=False)) == 1  # AT ends where AAAT ends: L = 4


# ---------------------------------------------------------------- CLI
def test_cli_amplicon_parser_and_primer_reader(sassy, capsys, tmp_path):
    from sassy_amd import cli
    primers = tmp_path / "primers.tsv"
    primers.write_bytes(b"# name\tfwd\trev\np1\tACGT\tGGCC\r\n\np2\tAARY\tNNAC\n")
    assert cli.load_primers(str(primers)) == [("p1", b"ACGT", b"GGCC"), ("p2", b"AARY", b"NNAC")]
    bad = tmp_path / "bad.tsv"
    bad.write_bytes(b"p1\tACGT\n")
    with pytest.raises(SystemExit) as e:
        cli.load_primers(str(bad))
    assert "bad.tsv:1" in str(e.value)
    for argv, word in ((["amplicon", str(primers), "-k", "1", "--min-len", "10", "--max-len", "20"], "FASTX"),
                       (["amplicon", str(primers), "x.fa", "--min-len", "10", "--max-len", "20"], "-k"),
                       (["amplicon", str(primers), "x.fa", "-k", "1", "--max-len", "20"], "--min-len"),
                       (["amplicon", str(primers), "x.fa", "-k", "255", "--min-len", "10", "--max-len", "20"], "0 <= k <= 254"),
                       (["amplicon", str(primers), "x.fa", "-k", "1", "--min-len", "0", "--max-len", "20"], "--min-len <= --max-len"),
                       (["amplicon", str(primers), "x.fa", "-k", "1", "--min-len", "30", "--max-len", "20"], "--min-len <= --max-len"),
                       (["amplicon", str(primers), "x.fa", "-k", "1", "--min-len", "1", "--max-len", str((1 << 24) + 1)], "2^24"),
                       (["amplicon", str(primers), "x.fa", "-k", "1", "--min-len", "1", "--max-len", "9", "-a", "ascii"], "invalid choice")):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert word in capsys.readouterr().err, argv


def test_cli_amplicon_row_writer_on_canned_records():
    from sassy_amd import cli
    pairs = [("p1", b"ACGT", b"GGCC"), ("p2", b"AARY", b"NNAC")]
    text = b"ACGTAAAAGGCCRYTT"
    recs = np.array([(0, 12, 0, 0, 0, 1, 0), (4, 16, 1, 1, 2, 0, 0)], dtype=aref.DTYPE)
    assert cli.AMPLICON_HEADER == "pair_id\ttext_id\tstrand\tstart\tend\tlength\tfwd_cost\trev_cost\n"
    assert cli.amplicon_rows(pairs, "chr1", recs) == ["p1\tchr1\t+\t0\t12\t12\t0\t1\n", "p2\tchr1\t-\t4\t16\t12\t2\t0\n"]
    assert cli.amplicon_rows(pairs, "chr1", recs, "iupac", text) == ["p1\tchr1\t+\t0\t12\t12\t0\t1\tACGTAAAAGGCC\n",
                                                                      "p2\tchr1\t-\t4\t16\t12\t2\t0\tAARYGGCCTTTT\n"]
    assert cli.product_bytes("dna", b"ACGTRacgt", 0, 9, 1) == b"tgcaRACGT"  # Dna complements upper-case ACGT only
    assert cli.product_bytes("iupac", b"ACGTRacgt", 0, 9, 1) == b"acgtYACGT"
    assert cli.amplicon_rows(pairs, "t", np.zeros(0, dtype=aref.DTYPE)) == []
