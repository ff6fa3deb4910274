"""CPU-only: demultiplexing (sassy_hip_demux_reads, DeviceReads.demux, `split`) and the gather (sassy_hip_reads_select,
DeviceReads.select) -- what needs no device: the definition's helper on the cases written out by hand and against a brute force
in plain Python, the arithmetic of demux_step.h driven by a stand-alone host program under AddressSanitizer / UBSan, the step
header's and the unit's layout, the symbols, every refusal the C call can raise without a read batch, the CLI's parser."""
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

import demux_reads_ref as dref  # noqa: E402
from hamming_ref import relation_row  # noqa: E402

NAME = "sassy_hip_demux_reads"
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")
# the barcodes of the seeded mixed batch (tests/test_gpu_demux_reads.py uses the same): the first two at distance 2
MIXED_BARCODES = [b"ACGTACGT", b"ACGTACAA", b"TTGGCCAA", b"GGATTCCA"]
MIXED_SEED = 1


@pytest.fixture(scope="module")
def sassy():
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


# ---------------------------------------------------------------- the definition
def test_helper_reproduces_the_cases_written_out_by_hand():
    assert len(dref.HAND) == 7
    for case in dref.HAND:
        records, order, bounds, seqs, quals = dref.expected_demux("dna", [case["seq"]], case["barcodes"], **case["call"])
        assert tuple(records[0].tolist()) == case["record"] + (0,), (case["name"], records)
        assert seqs == [case["kept"]] and quals == [None] and order.tolist() == [0], case["name"]
        B = len(case["barcodes"])
        label = case["record"][0] if case["record"][0] >= 0 else B
        assert bounds.tolist() == [0] * (label + 1) + [1] * (B + 1 - label), case["name"]
    by_name = {c["name"]: c for c in dref.HAND}
    assert by_name["a tie is unassigned under min_delta 1"]["seq"] == by_name["a tie goes to the smaller index under min_delta 0"]["seq"]
    assert by_name["no window"]["record"][1] == 0xFFFFFFFF


def _brute(profile, seq, barcodes, k, min_delta, at, end3):
    """The definition barcode by barcode in plain Python (no numpy): (sample, best, cost, second, n_best) and the label."""
    m, B, la = len(barcodes[0]), len(barcodes), len(seq)
    if at + m > la:
        return (-1, 0xFFFFFFFF, 255, 255, 0), B
    w = la - at - m if end3 else at
    costs = [sum(1 for i in range(m) if not relation_row(profile, bc[i])[seq[w + i]]) for bc in barcodes]
    cost = min(costs)
    best = costs.index(cost)
    second = min([c for j, c in enumerate(costs) if j != best], default=m + 1)
    assigned = cost <= k and second - cost >= min_delta
    return (best if assigned else -1, best, cost, second, costs.count(cost)), best if assigned else B


def test_helper_against_a_brute_force_on_random_reads():
    rnd = random.Random(11)
    letters = {"dna": b"ACGT", "iupac": b"ACGTNUNRYacgtn-X"}
    for profile in ("dna", "iupac"):
        assigned = ties = 0
        for _ in range(30):
            m, B = rnd.choice((1, 3, 8, 13)), rnd.choice((1, 2, 5, 9))
            barcodes = [bytes(rnd.choice(letters[profile]) for _ in range(m)) for _ in range(B)]
            at, end3, clip = rnd.randrange(4), rnd.random() < 0.5, rnd.random() < 0.7
            k, min_delta = rnd.choice((0, 1, 2, 64)), rnd.choice((0, 1, 2))
            reads = []
            for _ in range(10):
                la = rnd.randrange(40)
                seq = bytearray(rnd.choice(letters[profile]) for _ in range(la))
                if la >= at + m and rnd.random() < 0.8:
                    w = la - at - m if end3 else at
                    seq[w:w + m] = rnd.choice(barcodes)
                    if rnd.random() < 0.5:
                        seq[w + rnd.randrange(m)] = rnd.choice(letters[profile])
                reads.append((bytes(seq), bytes(rnd.randrange(33, 75) for _ in range(la))))
            records, order, bounds, seqs, quals = dref.expected_demux(profile, reads, barcodes, k=k, min_delta=min_delta, at=at, end3=end3, clip=clip)
            want = [_brute(profile, s, barcodes, k, min_delta, at, end3) for s, _ in reads]
            assert [tuple(r.tolist())[:5] for r in records] == [w[0] for w in want], (profile, barcodes, reads)
            labels = [w[1] for w in want]
            by_label = sorted(range(len(reads)), key=lambda r: (labels[r], r))
            assert order.tolist() == by_label and records["index"][by_label].tolist() == list(range(len(reads)))
            assert bounds.tolist() == [sum(1 for l in labels if l < s) for s in range(B + 2)]
            for j, r in enumerate(by_label):
                s, q = reads[r]
                lo, hi = 0, len(s)
                if labels[r] < B and clip:
                    lo, hi = (0, len(s) - at - m) if end3 else (at + m, len(s))
                assert (seqs[j], quals[j]) == (s[lo:hi], q[lo:hi])
            assigned += sum(1 for l in labels if l < B)
            ties += int((records["n_best"] > 1).sum())
        assert assigned > 60 and ties > 10, (profile, assigned, ties)


def test_the_seeded_mixed_batch_holds_all_five_groups():
    """The batch the GPU tests demultiplex is non-trivial by the helper alone: each group holds at least a tenth of the reads."""
    for n in (1023, 2049):
        reads = dref.mixed_batch(n, MIXED_SEED, MIXED_BARCODES)
        records = dref.expected_demux("dna", reads, MIXED_BARCODES, k=1, min_delta=1)[0]
        g = dref.groups(records, 1)
        assert sum(g.values()) == n and all(v * 10 >= n for v in g.values()), g
    assert sum(a != b for a, b in zip(*MIXED_BARCODES[:2])) == 2


def test_select_helper_and_layout():
    reads = [(b"ACGT", b"IIII"), (b"", b""), (b"A" * 70, b"#" * 70)]
    got = dref.expected_select(reads, [2, 0, 0, 1], begins=[64, 1, 0, 0], lens=[6, 2, 4, 0])
    assert got == [(b"AAAAAA", b"######"), (b"CG", b"II"), (b"ACGT", b"IIII"), (b"", b"")]
    assert dref.expected_select(reads, [2, 1]) == [reads[2], reads[1]]
    text, qual, starts, rem, longest = dref.layout([s for s, _ in reads], [q for _, q in reads])
    assert len(text) == 64 + 0 + 128 + 64 and starts.tolist() == [0, 64, 64] and rem.tolist() == [4, 70, 6] and longest == 70
    assert text[:4] == b"ACGT" and text[4:64] == bytes(60) and qual[64:134] == b"#" * 70 and text[-64:] == bytes(64)


# ---------------------------------------------------------------- the step header
MS = (1, 8, 31, 32, 33, 63, 64)
ATS = list(range(16)) + [63, 64, 127, 128, 447, 448]
BS = (1, 2, 63, 64, 65)


def test_step_arithmetic_against_a_byte_wise_brute_force_under_sanitizers(tmp_path):
    """tests/c/demux_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: demux_step.h as the kernels call it, a lane simulated, against a byte-wise brute force."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "demux_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "c", "demux_step_driver.cc")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    fields = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}
    # per profile, barcode length, place, end and barcode count: the read lengths at + m - 1, at + m, at + m + 1, 0 and 512
    per = sum(sum(1 for la in (at + m - 1, at + m, at + m + 1, 0, 512) if la <= 512) for m in MS for at in ATS if at + m <= 512)
    assert fields["cases"] == 2 * 2 * len(BS) * per, fields
    assert fields["refusals"] == 25, fields   # 16 refusals, the count, the length, the barcodes' null, `at` and Ascii twice, the outputs three times, 2 x ok
    assert fields["assigned"] * 10 > fields["cases"] and fields["ties"] > 0 and fields["no_window"] * 10 > fields["cases"], fields
    assert fields["reductions"] == 2000 and fields["blocks"] > 10000, fields


def test_step_header_is_free_of_hip_and_the_driver_stands_alone():
    src = open(os.path.join(CSRC, "demux_step.h")).read()
    code = re.sub(r"//.*", "", src)
    assert "#include <hip" not in src and "hipStream" not in src and "getenv" not in src
    assert "__builtin_amdgcn" not in src and "__HIP_DEVICE_COMPILE__" not in src and "asm" not in code and "switch" not in code
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>", '#include "trim_step.h"']
    for fn in ("dmx_refusal", "dmx_encode_barcode", "dmx_has_window", "dmx_window", "dmx_planes", "dmx_mismatches", "dmx_combine", "dmx_assigned",
               "dmx_label", "dmx_clip", "dmx_record", "dmx_lower_bound", "dmx_key_bits"):
        assert re.search(r"\b" + fn + r"\s*\(", src), fn
    # the relation is not restated: the row code and the mismatch word are the siblings'
    assert "ovl_mismatch_word<P, IUPAC>(" in code and "pairs_row_code(" in code and "ham_iupac_nib" not in code and ">> 1) & 3" not in code
    # the combine and the assignment are branch-free
    body = src[src.index("SASSY_HAM_HD DmxBest dmx_combine("):src.index("// the key of the sort")]
    assert "if (" not in body and "&&" not in re.sub(r"//.*", "", body) and "||" not in re.sub(r"//.*", "", body)
    driver = open(os.path.join(ROOT, "tests", "c", "demux_step_driver.cc")).read()
    assert "int main(" in driver and "#include <hip" not in driver and "__global__" not in driver and "demux_step.h" in driver


def test_source_layout():
    """The entry points live in demux_reads.hip with three kernels, no inline assembly, no atomics, no switch and no
    environment; the sort is rocPRIM's; the layout scan and the write kernel are the siblings', with one definition each."""
    unit = open(os.path.join(CSRC, "demux_reads.hip")).read()
    code = re.sub(r"//.*", "", unit)
    assert "int " + NAME + "(" in unit and "int sassy_hip_reads_select(" in unit
    assert "asm" not in code and "getenv" not in code and "atomic" not in code and "switch" not in code
    for kernel in ("demux_assign_kernel", "demux_bounds_kernel", "demux_place_kernel"):
        assert len(re.findall(r"__global__[^;{]*\b" + kernel + r"\(", unit)) == 1, kernel
    assert code.count("__global__") == 3
    assert "rocprim::radix_sort_pairs(" in code and "dmx_refusal(" in code and "dmx_combine(" in code and "trm_window_block(" in code
    assert "reads_layout_windows(" in code and "write_windows(" in code and "reads_require_plain(" in code and "dmx_lower_bound(" in code
    shared = open(os.path.join(CSRC, "reads_call.hip")).read()
    assert len(re.findall(r"\nint reads_require_plain\(", shared)) == 1 and shared.count("reads_plain(") == 1   # the Dna look: one owner, called here
    assert "fastq_rec_" not in code and "reads_window_write_kernel<" not in code and "hipMemset(" not in code   # no scan, no write kernel of its own
    host = open(os.path.join(CSRC, "host_internal.h")).read()
    for decl in ("int write_windows(", "int reads_empty_buffers(", "int reads_layout_windows("):
        assert decl in host, decl
    trim = open(os.path.join(CSRC, "trim_reads.hip")).read()
    assert len(re.findall(r"\nint write_windows\(", trim)) == 1 and "template <bool SHIFTED, bool GATHER>" in trim
    for inst in ("<true, true>", "<false, true>", "<true, false>", "<false, false>"):
        assert "reads_window_write_kernel" + inst in trim, inst
    fastq = open(os.path.join(CSRC, "fastq_reads.hip")).read()
    assert len(re.findall(r"\nstruct \w+Source \{", fastq)) == 4                                  # the scan gained no source
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"demux_reads.hip"' in build and '"demux_step.h"' in build


# ---------------------------------------------------------------- the surface
def test_symbols_are_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    L = sassy.lib()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    for name in (NAME, "sassy_hip_reads_select"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
    assert re.search(r"#define SASSY_HIP_DEMUX_MAX_BARCODES\s+4096u\b", hdr) and sassy.DEMUX_MAX_BARCODES == 4096 and "DEMUX_MAX_BARCODES: u32 = 4096" in rust
    assert re.search(r"#define SASSY_HIP_DEMUX_END3\s+1u\b", hdr) and re.search(r"#define SASSY_HIP_DEMUX_KEEP_BARCODE\s+2u\b", hdr)
    assert (sassy.DEMUX_END3, sassy.DEMUX_KEEP_BARCODE) == (1, 2) and "DEMUX_END3: u32 = 1" in rust and "DEMUX_KEEP_BARCODE: u32 = 2" in rust
    assert len(getattr(L, NAME).argtypes) == 13 and len(L.sassy_hip_reads_select.argtypes) == 7
    assert sassy.read_demux_dtype() == dref.DTYPE and sassy.read_demux_dtype().itemsize == 16
    assert "pub struct ReadDemux" in rust
    for attr in ("select", "nonempty", "demux"):
        assert hasattr(sassy.DeviceReads, attr), attr
    assert callable(sassy.demux_reads) and all(hasattr(sassy.Demuxed, a) for a in ("sample", "counts", "span"))
    doc = hdr[hdr.index("/* Demultiplexing"):hdr.index("int " + NAME)]
    for word in ("SORTED BY SAMPLE", "text_bytes == 64", "sassy_hip_reads_free", "second - cost >= min_delta", "the smallest j", "min_delta > 65",
                 "scan_launches = 8, or 9", "candidates = the assigned reads", "out_bounds is all zero", "SASSY_HIP_DEMUX_KEEP_BARCODE"):
        assert word in doc, word
    import inspect
    sig = inspect.signature(sassy.DeviceReads.demux).parameters
    assert [(k, v.default) for k, v in list(sig.items())[3:]] == [("k", 1), ("min_delta", 1), ("at", 0), ("end3", False), ("clip", True), ("with_records", False)]
    assert list(inspect.signature(sassy.DeviceReads.select).parameters)[1:4] == ["src", "begins", "lens"]


def test_searcher_gained_no_public_method(sassy):
    """The new surface is DeviceReads' and the module's: Searcher and its base classes have the public methods they had."""
    import inspect
    import call_catalogue as cc
    exempt = ("set_", "with_", "get_", "enable_", "_")
    inherited = [name for base in sassy.Searcher.__mro__[1:] if base is not object
                 for name, f in vars(base).items() if inspect.isfunction(f) and not name.startswith(exempt)]
    assert inherited == ["trim_reads"], inherited
    own = [name for name, f in vars(sassy.Searcher).items() if inspect.isfunction(f) and not name.startswith(exempt)]
    assert len(own) == 38 and set(own) >= {m for e in cc.ENTRIES for m in e.methods if not m.startswith(exempt)}, len(own)
    assert not any("demux" in name or "select" in name for name in dir(sassy.Searcher))


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal the C call can raise without a read batch, with its code and a message that names the reason, in their
    order, in a child that sees no device.  The refusals that read the batch are the same function's next lines: the driver
    above walks them, the GPU tests raise them."""
    code = r'''
import ctypes as C, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
FAKE = 0x7000000   # a batch pointer that is never read: every refusal below comes before the batch is looked at
def call(s, barcodes=(b"ACGT", b"TTAA"), reads=FAKE, blen=None, n=None, at=0, k=1, delta=1, flags=0, s_null=False, null_at=None, array=True):
    nb = len(barcodes)
    ptrs = (C.c_char_p * max(nb, 1))(*[None if i == null_at else b for i, b in enumerate(barcodes)])
    out = C.c_void_p(7)
    bounds = (C.c_uint64 * 5000)()
    rc = L.sassy_hip_demux_reads(None if s_null else s._h, reads, ptrs if array else None, len(barcodes[0]) if blen is None else blen,
                                 nb if n is None else n, at, k, delta, flags, None, None, bounds, C.byref(out))
    return rc, L.sassy_hip_last_error().decode(), out.value
def refused(s, want, word, **kw):
    rc, msg, out = call(s, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg and out is None, (rc, msg, want, word, out)
dna, iupac = sassy_amd.Searcher("dna", rc=False), sassy_amd.Searcher("iupac", rc=True)
everything = dict(flags=4, delta=66, n=0, blen=0, array=False, at=600, reads=None)   # each refusal hides the ones behind it
refused(dna, EINVAL, "demux_reads() must not be null", s_null=True, **everything)
refused(dna, EINVAL, "SASSY_HIP_DEMUX_END3 and SASSY_HIP_DEMUX_KEEP_BARCODE only", **everything)
for flags in (4 | 3, 4, 1 << 20, sassy_amd.KEEP_QUALITY << 8 | 1):
    refused(dna, EINVAL, "SASSY_HIP_DEMUX_END3 and SASSY_HIP_DEMUX_KEEP_BARCODE only", flags=flags)
everything.pop("flags")
refused(iupac, EINVAL, "min_delta must be <= 65 (got 66)", **everything)
everything.pop("delta")
refused(dna, EINVAL, "1 .. 4096 barcodes (SASSY_HIP_DEMUX_MAX_BARCODES; got 0)", **everything)
everything["n"] = 4097
refused(dna, EINVAL, "1 .. 4096 barcodes (SASSY_HIP_DEMUX_MAX_BARCODES; got 4097)", **everything)
everything.pop("n")
refused(dna, EINVAL, "barcode_len must be 1 .. 64 (got 0)", **everything)
everything["blen"] = 65
refused(dna, EINVAL, "barcode_len must be 1 .. 64 (got 65)", **everything)
everything.pop("blen")
ascii_ = sassy_amd.Searcher("ascii", rc=False)
refused(ascii_, EINVAL, "must not be null (barcode 0)", **everything)
everything.pop("array")
refused(ascii_, EINVAL, "must not be null (barcode 1)", null_at=1, **everything)
refused(ascii_, EINVAL, "at + barcode_len = 604 reaches past", **everything)
refused(ascii_, EINVAL, "at + barcode_len = 513 reaches past", at=509, reads=None)
for alphabet in ("ascii", "ascii_ci"):
    refused(sassy_amd.Searcher(alphabet, rc=False), EINVAL, "use a dna or an iupac searcher", at=508, reads=None)
refused(sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang", reads=None)
refused(sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match", reads=None)
refused(sassy_amd.Searcher("dna", rc=False).with_max_n_frac(0.2), EUNSUPPORTED, "demux_reads does not take max_n_frac", reads=None)
refused(dna, EINVAL, "demux_reads() must not be null", reads=None)
refused(dna, EINVAL, "demux_reads() must not be null", reads=None, flags=3, delta=0, k=1 << 40)
# the select: its pointers
out = C.c_void_p(7)
assert L.sassy_hip_reads_select(None, None, None, None, 0, None, C.byref(out)) == EINVAL and out.value is None
assert "reads_select() must not be null" in L.sassy_hip_last_error().decode()
assert L.sassy_hip_reads_select(FAKE, None, None, None, 3, None, C.byref(out)) == EINVAL and "reads_select() must not be null" in L.sassy_hip_last_error().decode()
one = (C.c_uint64 * 1)(0)
assert L.sassy_hip_reads_select(FAKE, one, one, None, 0, None, C.byref(out)) == EINVAL and "given together" in L.sassy_hip_last_error().decode()
assert L.sassy_hip_reads_select(FAKE, one, None, None, 1 << 32, None, C.byref(out)) == -3 and "more than 2^32 - 1" in L.sassy_hip_last_error().decode()
# the Python call: lists go through from_sequences, which refuses before anything else and then needs the device
for args, word in ((([(b"AC\nGT", b"IIIII")], [b"ACGT"]), "sequence 0 holds a line end"), (([(b"ACGT", b"III")], [b"ACGT"]), "quality 0 has 3 bytes, its sequence 4"),
                   (([b"ACGT"], [b"ACGT"]), "no usable HIP device"), (([], [b"ACGT"]), "no usable HIP device")):
    try:
        sassy_amd.demux_reads(dna, *args)
    except sassy_amd.SassyHipError as e:
        assert word in str(e), (word, e)
    else:
        raise SystemExit(3)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


# ---------------------------------------------------------------- CLI
def test_cli_split_parser(sassy, capsys, tmp_path):
    from sassy_amd import cli
    import argparse
    ap = argparse.ArgumentParser()
    sp = cli.split_parser(ap.add_subparsers(dest="cmd"))
    args = sp.parse_args(["in.fq", "-f", "bc.fa", "-k", "1", "-o", "out"])
    assert (args.input, args.barcodes, args.k, args.outdir, args.mate, args.at, args.end3, args.min_delta, args.keep_barcode, args.alphabet, args.tsv) == \
        ("in.fq", "bc.fa", 1, "out", "", 0, False, 1, False, "dna", False)
    args = sp.parse_args(["in.fq", "-f", "bc.fa", "-k", "0", "-o", "out", "--mate", "r2.fq", "--at", "3", "--end3", "--min-delta", "2", "--keep-barcode",
                          "--alphabet", "iupac", "--tsv"])
    assert (args.mate, args.at, args.end3, args.min_delta, args.keep_barcode, args.alphabet, args.tsv) == ("r2.fq", 3, True, 2, True, "iupac", True)
    for argv in (["in.fq", "-k", "1", "-o", "out"], ["in.fq", "-f", "bc.fa", "-o", "out"], ["in.fq", "-f", "bc.fa", "-k", "1"],
                 ["in.fq", "-f", "bc.fa", "-k", "1", "-o", "out", "--alphabet", "ascii"]):
        with pytest.raises(SystemExit):
            sp.parse_args(argv)
    capsys.readouterr()
    fa = tmp_path / "bc.fa"
    fa.write_bytes(b">s1 first\nACGT\n>s2\nTTAA\n")
    base = ["split", "in.fq", "-f", str(fa), "-o", str(tmp_path / "out")]
    for argv in (["-k", "-1"], ["-k", "1", "--at", "-1"], ["-k", "1", "--min-delta", "66"]):
        with pytest.raises(SystemExit):
            cli.main(base + argv)
        assert "split takes -k >= 0" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(base + ["-k", "1", "--at", "509"])
    assert "reach past 512" in capsys.readouterr().err
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b">s1\nACGT\n>s2\nTTA\n")
    with pytest.raises(SystemExit):
        cli.main(["split", "in.fq", "-f", str(bad), "-k", "1", "-o", str(tmp_path / "out")])
    assert "barcodes of one length" in capsys.readouterr().err
    assert cli.split_names([("s1 first", b"ACGT"), ("s2", b"TTAA")]) == ["s1", "s2"]
    for ids in (["a", "a"], ["unassigned"], ["x/y"], [""], ["s_2"]):
        with pytest.raises(SystemExit):
            cli.split_names([(i, b"ACGT") for i in ids])
    records = np.array([(1, 1, 0, 4, 1, 0), (-1, 0, 2, 2, 2, 1), (-1, 0xFFFFFFFF, 255, 255, 0, 2)], dtype=dref.DTYPE)
    assert cli.split_rows(["r0 x", "r1", "r2"], ["s1", "s2", "unassigned"], records) == \
        ["r0 x\ts2\t1\t0\t4\t1\n", "r1\tunassigned\t0\t2\t2\t2\n", "r2\tunassigned\t-1\t255\t255\t0\n"]
    assert cli.SPLIT_HEADER.count("\t") == 5
    assert not os.path.exists(tmp_path / "out")   # nothing above got as far as the device or the files
