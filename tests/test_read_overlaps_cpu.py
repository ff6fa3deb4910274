"""CPU-only: the paired-end overlap call (sassy_hip_read_overlaps, Searcher.read_overlaps, `overlap`) -- what needs no device:
the definition's helper on the cases written out by hand and against a brute force, overlap_trims, the arithmetic of
overlap_step.h driven by a stand-alone host program under AddressSanitizer / UBSan, the step header's and the unit's layout,
the symbol, every refusal that the C call can raise without a read batch (the ones that read a batch's numbers: through the
step header's function in the driver, and on the device in tests/test_gpu_read_overlaps.py), the loud failure without a device,
the FASTQ bytes of from_sequences, the pair reader's cuts, the CLI's parser and row writer."""
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
sys.path.insert(0, ROOT)

import read_overlaps_ref as oref  # noqa: E402
from hamming_ref import relation_row  # noqa: E402
import oracle  # noqa: E402

NAME = "sassy_hip_read_overlaps"
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


@pytest.fixture(scope="module")
def sassy():
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


# ---------------------------------------------------------------- the definition
def test_helper_reproduces_the_two_cases_written_out_by_hand():
    for case in oref.HAND:
        assert oracle.reverse_complement("dna", case["r2"]) == case["b"]
        rec = oref.expected_overlaps("dna", [case["r1"]], [case["r2"]], case["min_overlap"], 0, 0)[0]
        assert tuple(rec.tolist()) == case["record"], (case, rec)
        assert oref.trims(rec, len(case["r1"]), len(case["r2"])) == case["trims"]
    # an empty read on either side, and a pair without an accepted offset: all four fields zero
    got = oref.expected_overlaps("dna", [b"", b"ACGT", b"AAAAAAAA"], [b"ACGT", b"", b"CCCCCCCC"], 1, 0, 0)
    assert got.tolist() == [(0, 0, 0, 0)] * 3 and got.dtype.itemsize == 16


def _brute(profile, r1, r2, min_overlap, k, permille):
    """The definition in three lines of plain Python per offset (no numpy, no planes)."""
    b, best, n = oracle.reverse_complement(profile, r2), None, 0
    for d in range(-(len(b) - 1), len(r1)) if r1 and b else ():
        rows = range(max(0, d), min(len(r1), d + len(b)))
        mm = sum(not relation_row(profile, r1[i])[b[i - d]] for i in rows)
        if len(rows) >= min_overlap and mm <= k and mm * 1000 <= permille * len(rows):
            n += 1
            if best is None or mm * best[1] < best[2] * len(rows) or (mm * best[1] == best[2] * len(rows) and (len(rows), d) > (best[1], best[0])):
                best = (d, len(rows), mm)
    return (best[0], best[1], best[2], n) if best else (0, 0, 0, 0)


def test_helper_against_a_brute_force_on_random_pairs():
    rnd = random.Random(5)
    letters = {"dna": b"ACGT", "iupac": b"ACGTNUNURYacgtn-X"}
    for profile in ("dna", "iupac"):
        for _ in range(300):
            la, lb = rnd.randrange(21), rnd.randrange(21)
            r1 = bytes(rnd.choice(letters[profile]) for _ in range(la))
            r2 = bytes(rnd.choice(letters[profile]) for _ in range(lb))
            if la and lb and rnd.random() < 0.5:  # a planted overlap, so that something is accepted at small k
                ov = rnd.randrange(1, min(la, lb) + 1)
                r2 = oracle.reverse_complement(profile, r1[la - ov:] + oracle.reverse_complement(profile, r2)[ov:])
            mo, k, pm = rnd.randrange(1, 8), rnd.choice((0, 1, 2, 512)), rnd.choice((0, 100, 250, 1000))
            got = tuple(oref.expected_overlaps(profile, [r1], [r2], mo, k, pm)[0].tolist())
            assert got == _brute(profile, r1, r2, mo, k, pm), (profile, r1, r2, mo, k, pm)
    # under Iupac both sides see N and U: U matches as T and is its own complement; N matches everything
    assert oracle.reverse_complement("iupac", b"UN") == b"NU"
    assert tuple(oref.expected_overlaps("iupac", [b"AAAT"], [b"AUUU"], 4, 0, 0)[0].tolist()) == (0, 0, 0, 0)   # b = UUUA: T against A
    assert tuple(oref.expected_overlaps("iupac", [b"TTTA"], [b"NUUU"], 4, 0, 0)[0].tolist()) == (0, 4, 0, 1)   # b = UUUN


def test_overlap_trims_on_hand_cases(sassy):
    dt = sassy.read_overlap_dtype()
    assert dt == oref.DTYPE and dt.itemsize == 16

    def rec(*fields):
        return np.array([fields], dtype=dt)[0]

    assert sassy.overlap_trims(rec(3, 6, 0, 1), 9, 9) == (12, 9, 9)          # d > 0: the fragment is longer than a read
    assert sassy.overlap_trims(rec(0, 9, 1, 2), 9, 12) == (12, 9, 12)        # d == 0 and b longer: insert = d + lb
    assert sassy.overlap_trims(rec(0, 9, 0, 1), 12, 9) == (12, 12, 9)
    assert sassy.overlap_trims(rec(-2, 6, 0, 1), 8, 8) == (6, 6, 6)          # read-through: both tails are adapter
    assert sassy.overlap_trims(rec(-5, 4, 0, 1), 4, 20) == (4, 4, 15)        # ... a short first read: keep1 = la
    assert sassy.overlap_trims(rec(0, 0, 0, 0), 8, 11) == (0, 8, 11)         # no overlap
    for case in oref.HAND:
        assert sassy.overlap_trims(rec(*case["record"]), len(case["r1"]), len(case["r2"])) == case["trims"]
        assert sassy.overlap_trims(rec(*case["record"]), len(case["r1"]), len(case["r2"])) == oref.trims(case["record"], len(case["r1"]), len(case["r2"]))


# ---------------------------------------------------------------- the step header
def _driver(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "overlap_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "c", "overlap_step_driver.cc")])
    return exe


def test_step_arithmetic_against_a_byte_wise_brute_force_under_sanitizers(tmp_path):
    """tests/c/overlap_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: the planes and the shifted-plane mismatch count at every offset of every length 0 .. 130,
    191 .. 193, 511 and 512, the range of offsets a call looks at, the record as the kernel finds it against the rule as
    written, every refusal in its order.  Its complement of every byte is the oracle's."""
    exe = _driver(tmp_path)
    r = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    fields = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}
    # per profile: a length against the 16 border lengths both ways -- 14 of the 134 lengths up to 193 are border lengths and meet
    # themselves once; 511 and 512 meet the 14 borders up to 193 and themselves --, each length against itself and a random one,
    # and 512 x 511 both ways at the end
    assert fields["pairs"] == 2 * (14 * 31 + 120 * 32 + 2 * 29 + 136 * 2 + 2), fields
    assert fields["offsets"] > 3000000 and fields["bests"] == 6 * fields["pairs"] and fields["refusals"] == 22
    r = subprocess.run([exe, "complement"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    tables = dict(line.split() for line in r.stdout.splitlines())
    for profile in ("dna", "iupac"):
        want = b"".join(oracle.reverse_complement(profile, bytes([c])) for c in range(256))
        assert bytes.fromhex(tables[profile]) == want, profile


def test_step_header_is_free_of_hip_and_the_driver_stands_alone():
    src = open(os.path.join(CSRC, "overlap_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "getenv" not in src
    assert "__builtin_amdgcn" not in src and "__HIP_DEVICE_COMPILE__" not in src and "asm" not in re.sub(r"//.*", "", src)
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>", '#include "pairs_step.h"',
                                                                         '#include "reads_gate.h"']
    for fn in ("ovl_refusal", "ovl_complement", "ovl_row_code", "ovl_offsets", "ovl_overlap", "ovl_shifted_word", "ovl_mismatch_word", "ovl_accepts",
               "ovl_better", "ovl_combine", "ovl_words"):
        assert re.search(r"\b" + fn + r"\s*\(", src), fn
    assert "pairs_row_code(" in src and "kOvlMaxLen = 512" in src      # the encoding is pairs_step.h's, the limit the header's
    driver = open(os.path.join(ROOT, "tests", "c", "overlap_step_driver.cc")).read()
    assert "int main(" in driver and "#include <hip" not in driver and "__global__" not in driver and "overlap_step.h" in driver
    assert "ham_match(" in driver                                        # the brute force counts with the family's relation


def test_source_layout():
    """The entry point lives in read_overlaps.hip, one kernel, no inline assembly and no environment; the refusals are the
    step header's function and come before the device; the Dna look is reads_plain, once per handle."""
    unit = open(os.path.join(CSRC, "read_overlaps.hip")).read()
    code = re.sub(r"//.*", "", unit)
    assert "int " + NAME + "(" in unit and "asm" not in code and "getenv" not in code
    assert len(re.findall(r"__global__[^;{]*\bread_overlaps_kernel\(", unit)) == 1
    entry = unit[unit.index("int " + NAME + "("):]
    assert entry.index("ovl_refusal(") < entry.index("SASSY_NO_TICKETS") < entry.index("hamming_call(") < entry.index("overlaps_run(")
    assert unit.count("reads_require_plain(") == 1 and "for (const sassy_hip_Reads* r : {r1, r2})" in unit
    shared = open(os.path.join(CSRC, "reads_call.hip")).read()
    assert len(re.findall(r"\nint reads_require_plain\(", shared)) == 1 and shared.count("reads_plain(") == 1   # the Dna look: one owner, called here
    for name in ("ovl_row_code(", "ovl_shifted_word(", "ovl_mismatch_word<", "ovl_accepts(", "ovl_combine(", "ovl_offsets(", "__ballot(", "__shfl_xor("):
        assert name in unit, name
    # every word count ovl_words can return is instantiated
    for w in (2, 4, 6, 8, 16):
        assert "read_overlaps_kernel<%d, IUPAC>" % w in unit
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"read_overlaps.hip"' in build and '"overlap_step.h"' in build


# ---------------------------------------------------------------- the surface
def test_symbol_is_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    L = sassy.lib()
    assert re.search(r"\b" + NAME + r"\s*\(", hdr) and "} sassy_hip_ReadOverlap;" in hdr
    assert re.search(r"#define SASSY_HIP_OVERLAP_MAX_LEN\s+512u\b", hdr) and sassy.OVERLAP_MAX_LEN == 512
    assert hasattr(L, NAME) and NAME in sassy.EXPORTED_SYMBOLS
    assert getattr(L, NAME).restype is not None and len(getattr(L, NAME).argtypes) == 8
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    assert re.search(r"fn\s+" + NAME + r"\s*\(", block) and "pub struct ReadOverlap" in rust
    assert hasattr(sassy.Searcher, "read_overlaps") and hasattr(sassy.DeviceReads, "from_sequences")
    from sassy_amd import fastx
    assert hasattr(fastx, "read_fastq_pair_device_batches")
    doc = hdr[hdr.index("/* Paired-end read overlap"):hdr.index("int " + NAME)]
    for word in ("mm * 1000 <= max_permille * ov", "larger d", "n_accepted", "U is its own complement", "iupac searcher", "not capped at 254"):
        assert word in doc, word


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal the C call can raise without a read batch, with its code and a message that names the reason, in a child
    that sees no device (no batch can be made there: the parse itself needs the device).  The refusals that read a batch --
    record counts, device, the length limit, `out` -- are the same function's next lines: the driver above walks them, the GPU
    tests raise them.  Then the Python call: its own refusals, and the loud failure without a device."""
    code = r'''
import ctypes as C, numpy as np, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
out = np.zeros(4, dtype=sassy_amd.read_overlap_dtype())
FAKE = 0x7000000   # a batch pointer that is never read: every refusal below comes before the batches are looked at
def call(s, r1=FAKE, r2=FAKE, min_overlap=10, k=512, permille=200, flags=0, s_null=False):
    rc = L.sassy_hip_read_overlaps(None if s_null else s._h, r1, r2, min_overlap, k, permille, flags, out.ctypes.data)
    return rc, L.sassy_hip_last_error().decode()
def refused(s, want, word, **kw):
    rc, msg = call(s, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (rc, msg, want, word)
dna, iupac = sassy_amd.Searcher("dna", rc=False), sassy_amd.Searcher("iupac", rc=True)
refused(dna, EINVAL, "read_overlaps() must not be null", s_null=True)
for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.ALL_MINIMA, sassy_amd.TEXT_ON_DEVICE, sassy_amd.TEXT_UNCHANGED, sassy_amd.LINE_SPANS, 1 << 20):
    refused(dna, EINVAL, "read_overlaps takes no flags", flags=flags)
refused(dna, EINVAL, "min_overlap must be at least 1", min_overlap=0)
refused(iupac, EINVAL, "max_permille must be <= 1000 (got 1001)", permille=1001)
refused(iupac, EINVAL, "max_permille must be <= 1000", permille=0xFFFFFFFF)
for alphabet in ("ascii", "ascii_ci"):
    refused(sassy_amd.Searcher(alphabet, rc=False), EINVAL, "have no complement")
    refused(sassy_amd.Searcher(alphabet, rc=False), EINVAL, "iupac searcher")
refused(sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang")
refused(sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match")
refused(sassy_amd.Searcher("dna", rc=False).with_max_n_frac(0.2), EUNSUPPORTED, "read_overlaps does not take max_n_frac")
refused(dna, EINVAL, "read_overlaps() must not be null", r1=None)
refused(dna, EINVAL, "read_overlaps() must not be null", r2=None)
refused(iupac, EINVAL, "read_overlaps() must not be null", r1=None, r2=None, k=1 << 40)
# the Python call: lists go through DeviceReads.from_sequences, which refuses line ends before anything else and then needs the device
for args, word in ((([b"AC\nGT"], [b"ACGT"]), "sequence 0 holds a line end"), (([b"ACGT"], [b"ACGT", b"AC\rGT"]), "sequence 1 holds a line end"),
                   (([b"ACGT"], [b"ACGT"]), "no usable HIP device"), (([], []), "no usable HIP device")):
    try:
        dna.read_overlaps(*args)
    except sassy_amd.SassyHipError as e:
        assert word in str(e), (word, e)
    else:
        raise SystemExit(3)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_from_sequences_builds_minimal_fastq_and_refuses_line_ends(sassy):
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import fastq_ref
    seqs = [b"ACGT", b"", b"NNU-x", "acgt"]
    raw = sassy.fastq_from_sequences(seqs)
    assert raw == b"@\nACGT\n+\n\n@\n\n+\n\n@\nNNU-x\n+\n\n@\nacgt\n+\n\n"
    assert [(i, s, q) for i, s, q in fastq_ref.records(raw)] == [("", b"ACGT", b""), ("", b"", b""), ("", b"NNU-x", b""), ("", b"acgt", b"")]
    assert sassy.fastq_from_sequences([]) == b""
    for bad in ([b"AC\nGT"], [b"ACGT", b"\r"], [b"ACGT\n"]):
        with pytest.raises(sassy.SassyHipError, match="line end"):
            sassy.fastq_from_sequences(bad)


# ---------------------------------------------------------------- the pair reader
def _fills(data: bytes, step: int):
    """fill(view) over `data` that hands out at most `step` bytes a call."""
    state = {"at": 0}

    def fill(view):
        n = min(len(view), step, len(data) - state["at"])
        view[:n] = data[state["at"]:state["at"] + n]
        state["at"] += n
        return n
    return fill


def test_pair_reader_cuts_both_files_at_the_same_record(sassy):
    import fastq_ref
    from sassy_amd import fastx
    assert fastx.whole_records(8, 0, False) == 2 and fastx.whole_records(7, 5, False) == 1 and fastx.whole_records(7, 5, True) == 2
    assert fastx.whole_records(3, 0, True) == 0 and fastx.pair_cut(3, 5) == 3 and fastx.pair_cut(0, 5) == 0
    nl = np.array([2, 5, 7, 10, 13, 16, 18], dtype=np.int64)
    assert fastx.records_end(nl, 1, 21) == 11 and fastx.records_end(nl, 2, 21) == 21 and fastx.records_end(nl, 0, 21) == 0
    # two files whose records have different sizes, so the chunk borders fall at different records of each
    rnd = random.Random(3)
    n = 57
    f1 = b"".join(b"@a%d x\n%s\n+\n%s\n" % (i, b"ACGT" * rnd.randrange(0, 9), b"I" * rnd.randrange(i // (n - 1), 30)) for i in range(n))
    # (the last quality line is not empty: an empty one exists only with its line end, which one variant below cuts off)
    f2 = b"".join(b"@b%d\r\n%s\r\n+b%d\r\n%s\r\n" % (i, b"GGC" * rnd.randrange(0, 30), i, b"@" * rnd.randrange(0, 5)) for i in range(n))
    want1, want2 = fastq_ref.records(f1), fastq_ref.records(f2)
    for batch, step in ((64, 7), (200, 1000), (1000, 13), (1 << 20, 1 << 20)):
        for a, b in ((f1, f2), (f1[:-1], f2), (f2, f1[:-1])):          # (a last line without its line end)
            got1, got2, chunks = [], [], 0
            for c1, c2 in fastx.fastq_pair_chunks(_fills(a, step), _fills(b, step), batch):
                r1, r2 = fastq_ref.records(c1.tobytes()), fastq_ref.records(c2.tobytes())
                assert len(r1) == len(r2) > 0
                got1 += r1
                got2 += r2
                chunks += 1
            assert [x[:2] for x in got1] == [x[:2] for x in (want1 if a[:2] == b"@a" else want2)], (batch, step)
            assert [x[:2] for x in got2] == [x[:2] for x in (want2 if b[:2] == b"@b" else want1)], (batch, step)
            assert chunks > 1 or batch >= len(f1)
    # files that end with different record counts raise, wherever the chunk borders fall; so does a file that ends inside a record
    one = b"@a\nAC\n+\nII\n"
    for batch in (16, 30, 1 << 20):
        for a, b in ((one * 3, one * 2), (one * 2, one * 5), (one, b""), (b"", one)):
            with pytest.raises(ValueError, match="different record counts"):
                list(fastx.fastq_pair_chunks(_fills(a, 1000), _fills(b, 1000), batch))
        with pytest.raises(ValueError, match="inside a FASTQ record|different record counts"):
            list(fastx.fastq_pair_chunks(_fills(one * 2 + b"@a\nAC\n", 1000), _fills(one * 2 + b"@a\nAC\n", 1000), batch))
    assert list(fastx.fastq_pair_chunks(_fills(b"", 10), _fills(b"", 10), 64)) == []


# ---------------------------------------------------------------- CLI
def test_cli_overlap_parser_and_row_writer(sassy, capsys, tmp_path):
    from sassy_amd import cli
    import argparse
    ap = argparse.ArgumentParser()
    op = cli.overlap_parser(ap.add_subparsers(dest="cmd"))
    args = op.parse_args(["a.fq", "b.fq"])
    assert (args.r1, args.r2, args.min_overlap, args.k, args.max_permille, args.alphabet) == ("a.fq", "b.fq", 10, 512, 200, "dna")
    args = op.parse_args(["a.fq", "b.fq", "--min-overlap", "4", "-k", "0", "--max-permille", "0", "--alphabet", "iupac"])
    assert (args.min_overlap, args.k, args.max_permille, args.alphabet) == (4, 0, 0, "iupac")
    with pytest.raises(SystemExit):
        op.parse_args(["a.fq", "b.fq", "--alphabet", "ascii"])
    capsys.readouterr()
    for argv in (["--min-overlap", "0"], ["--max-permille", "1001"], ["-k", "-1"]):
        with pytest.raises(SystemExit):
            cli.main(["overlap", "a.fq", "b.fq"] + argv)
        assert "overlap takes --min-overlap >= 1" in capsys.readouterr().err
    assert cli.OVERLAP_HEADER == "id\toffset\toverlap\tmismatches\taccepted\tinsert\tkeep1\tkeep2\n"
    records = np.array([c["record"] for c in oref.HAND] + [(0, 0, 0, 0)], dtype=sassy.read_overlap_dtype())
    rows = cli.overlap_rows(["p0", "p1", "p2"], records, [9, 8, 5], [9, 8, 7])
    assert rows == ["p0\t3\t6\t0\t1\t12\t9\t9\n", "p1\t-2\t6\t0\t1\t6\t6\t6\n", "p2\t0\t0\t0\t0\t0\t5\t7\n"]
