"""CPU-only: the paired-end merge (sassy_hip_merge_pairs, Searcher.merge_pairs, `merge`) and the kept qualities
(SASSY_HIP_KEEP_QUALITY) -- what needs no device: the definition's helper on the three cases written out by hand and against a
brute force in plain Python, the arithmetic of merge_step.h driven by a stand-alone host program under AddressSanitizer /
UBSan, the step header's and the unit's layout, the symbols, every refusal the C call can raise without a read batch, the
FASTQ bytes of from_sequences with qualities, reads_to_fastq's slicing, the CLI's parser."""
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

import fastq_ref  # noqa: E402
import merge_pairs_ref as mref  # noqa: E402
import read_overlaps_ref as oref  # noqa: E402
import oracle  # noqa: E402

NAME = "sassy_hip_merge_pairs"
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


@pytest.fixture(scope="module")
def sassy():
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


# ---------------------------------------------------------------- the definition
def test_helper_reproduces_the_three_cases_written_out_by_hand():
    assert len(mref.HAND) == 3 and mref.HAND_CALL == dict(min_overlap=4, k=1, max_permille=200)
    for case in mref.HAND:
        records, seqs, quals = mref.expected_merge("dna", [(case["r1"], case["q1"])], [(case["r2"], case["q2"])], **mref.HAND_CALL)
        assert tuple(records[0].tolist()) == case["record"], (case, records)
        assert (seqs[0], quals[0]) == (case["merged"], case["quality"]), (case, seqs, quals)
        assert len(seqs[0]) == oref.trims(case["record"], len(case["r1"]), len(case["r2"]))[0]  # the merged length is overlap_trims' insert
    # the second case's column 4 by hand: T at '+' (10) against C at 'I' (40)
    assert mref.HAND[1]["quality"][4] == 33 + 30 == ord("?")


def test_helper_records_are_the_overlap_helpers(sassy):
    rng = np.random.default_rng(3)
    pairs1, pairs2 = [], []
    for la, lb, d in ((20, 20, 5), (30, 12, 9), (12, 30, -4), (9, 9, 0), (15, 15, 10), (0, 10, 0), (10, 0, 0), (10, 10, 0)):
        r1, r2 = oref.planted_pair(rng, "dna", la, lb, d, subs=int(rng.integers(0, 2)))
        if (la, lb, d) == (10, 10, 0):
            r1, r2 = b"AAAAAAAAAA", b"AAAAAAAAAA"  # b = TTTTTTTTTT: nothing is accepted
        pairs1.append((r1, bytes(rng.integers(33, 75, la).astype(np.uint8))))
        pairs2.append((r2, bytes(rng.integers(33, 75, lb).astype(np.uint8))))
    for profile in ("dna", "iupac"):
        records, seqs, quals = mref.expected_merge(profile, pairs1, pairs2, 4, 2, 200)
        assert records.dtype == oref.DTYPE
        assert np.array_equal(records, oref.expected_overlaps(profile, [x[0] for x in pairs1], [x[0] for x in pairs2], 4, 2, 200))
        for rec, s, q, (r1, _), (r2, _) in zip(records, seqs, quals, pairs1, pairs2):
            assert len(s) == len(q) == oref.trims(rec, len(r1), len(r2))[0] == sassy.overlap_trims(rec, len(r1), len(r2))[0]
        assert [len(s) for s in seqs[-3:]] == [0, 0, 0] and all(len(s) for s in seqs[:5])


def _brute(profile, r1, q1, r2, q2, rec):
    """The definition column by column in plain Python (no numpy)."""
    d, ov, _, n = rec
    if n == 0:
        return b"", b""
    b, qb = oracle.reverse_complement(profile, r2), q2[::-1]
    L = max(len(r1), d + len(b)) if d >= 0 else ov
    s, q = bytearray(), bytearray()
    for p in range(L):
        j = p - d
        in_a, in_b = p < len(r1), 0 <= j < len(b)
        if in_a and in_b:
            if r1[p] == b[j]:
                s.append(r1[p]), q.append(max(q1[p], qb[j]))
            else:
                s.append(b[j] if qb[j] > q1[p] else r1[p]), q.append(min(126, 33 + max(2, abs(q1[p] - qb[j]))))
        elif in_a:
            s.append(r1[p]), q.append(q1[p])
        else:
            s.append(b[j]), q.append(qb[j])
    return bytes(s), bytes(q)


def test_helper_against_a_brute_force_on_random_pairs():
    rnd = random.Random(11)
    letters = {"dna": b"ACGT", "iupac": b"ACGTNUNRYacgtn-X"}
    for profile in ("dna", "iupac"):
        merged = 0
        for _ in range(300):
            la, lb = rnd.randrange(25), rnd.randrange(25)
            r1 = bytes(rnd.choice(letters[profile]) for _ in range(la))
            r2 = bytes(rnd.choice(letters[profile]) for _ in range(lb))
            if la and lb and rnd.random() < 0.7:
                ov = rnd.randrange(1, min(la, lb) + 1)
                r2 = oracle.reverse_complement(profile, r1[la - ov:] + oracle.reverse_complement(profile, r2)[ov:])
            q1, q2 = bytes(rnd.randrange(256) for _ in range(la)), bytes(rnd.randrange(256) for _ in range(len(r2)))
            mo, k, pm = rnd.randrange(1, 6), rnd.choice((0, 1, 2, 512)), rnd.choice((0, 100, 250, 1000))
            records, seqs, quals = mref.expected_merge(profile, [(r1, q1)], [(r2, q2)], mo, k, pm)
            assert (seqs[0], quals[0]) == _brute(profile, r1, q1, r2, q2, tuple(records[0].tolist())), (profile, r1, r2, mo, k, pm)
            merged += bool(seqs[0])
        assert merged > 100


def test_layout_helper_is_the_parse_helpers():
    seqs = [b"ACGT", b"", b"A" * 64, b"C" * 65, b"", b""]
    starts, lens, buf = mref.layout_of(seqs)
    raw = b"".join(b"@\n" + s + b"\n+\n" + s.lower() + b"\n" for s in seqs)
    reads = fastq_ref.parse(raw)
    assert starts.tolist() == [r.seq_start for r in reads] == [0, 64, 64, 128, 256, 256] and lens.tolist() == [4, 0, 64, 65, 0, 0]
    assert buf.tobytes() == fastq_ref.layout(reads) and buf.size == 256 + 64
    assert mref.quality_layout(raw).tobytes() == fastq_ref.layout(reads).lower()  # (the qualities are the sequences in lower case)
    assert mref.layout_of([])[2].tobytes() == bytes(64) and mref.layout_of([b"", b""])[2].tobytes() == bytes(64)


# ---------------------------------------------------------------- the step header
def test_step_arithmetic_against_a_byte_wise_brute_force_under_sanitizers(tmp_path):
    """tests/c/merge_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: the merged length and every 64-byte block as the write kernel builds it, at every offset that
    has an overlap, for every (la, lb) in 0 .. 70 and 127, 128, 129, 511, 512 against the border lengths, both profiles; all
    256 x 256 quality pairs through mrg_consensus with equal and unequal bytes; every refusal in its order."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "merge_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "c", "merge_step_driver.cc")])
    r = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    fields = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}
    # per profile: 71 x 71 pairs, and five long lengths against ten border lengths both ways
    assert fields["pairs"] == 2 * (71 * 71 + 5 * 10 * 2), fields
    # every offset of every pair of non-empty reads: la + lb - 1 of them
    small = sum(la + lb - 1 for la in range(1, 71) for lb in range(1, 71))
    long_ = sum(2 * (l + o - 1) for l in (127, 128, 129, 511, 512) for o in (1, 63, 64, 65, 127, 128, 129, 511, 512))
    assert fields["offsets"] == 2 * (small + long_), fields
    assert fields["columns"] > 64 * fields["offsets"] and fields["consensus"] == 7 * 65536 and fields["refusals"] == 21


def test_step_header_is_free_of_hip_and_the_driver_stands_alone():
    src = open(os.path.join(CSRC, "merge_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "getenv" not in src
    assert "__builtin_amdgcn" not in src and "__HIP_DEVICE_COMPILE__" not in src and "asm" not in re.sub(r"//.*", "", src)
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>", '#include "overlap_step.h"']
    for fn in ("mrg_length", "mrg_sources", "mrg_consensus", "mrg_refusal", "mrg_word"):
        assert re.search(r"\b" + fn + r"\s*\(", src), fn
    # the refusals and the complement are overlap_step.h's: called, not copied
    assert "ovl_refusal(c.ovl, gate)" in src and "ovl_complement(profile," in src and "'A' ? 'T'" not in src
    # the consensus is branch-free: selects on scalars, no `if`, no struct-valued ?:
    body = src[src.index("SASSY_HAM_HD MrgByte mrg_consensus("):src.index("// One column out of what covers it")]
    assert "if (" not in body and "&&" not in body and "||" not in body
    driver = open(os.path.join(ROOT, "tests", "c", "merge_step_driver.cc")).read()
    assert "int main(" in driver and "#include <hip" not in driver and "__global__" not in driver and "merge_step.h" in driver


def test_source_layout():
    """The entry point lives in merge_pairs.hip with one write kernel, no inline assembly, no atomics and no environment; the
    overlap is read_overlaps.hip's through one thin function; the scan is fastq_reads.hip's, with a second source of lengths;
    the copy kernel exists once and takes the line as a parameter."""
    unit = open(os.path.join(CSRC, "merge_pairs.hip")).read()
    code = re.sub(r"//.*", "", unit)
    assert "int " + NAME + "(" in unit and "asm" not in code and "getenv" not in code and "atomic" not in code
    assert len(re.findall(r"__global__[^;{]*\bmerge_write_kernel\(", unit)) == 1 and code.count("__global__") == 1
    assert "ovl_refusal" not in code and "mrg_refusal(" in code and "overlap_refused(" in code   # the refusals: called, not copied
    assert "overlaps_resident(" in code and "reads_layout_merged(" in code and "read_overlaps_kernel" not in code
    assert "ham_text_of(" in code and "ham_rem(" in code and "mrg_word(" in code and "hipMemset(" not in code
    assert "reads_plain(" not in code                                   # the Dna look stays where it is
    host = open(os.path.join(CSRC, "host_internal.h")).read()
    for decl in ("int overlaps_resident(", "int reads_layout_merged(", "int overlap_refused("):
        assert decl in host, decl
    overlaps = open(os.path.join(CSRC, "read_overlaps.hip")).read()
    assert overlaps.count("reads_require_plain(") == 1 and "int overlaps_resident(" in overlaps
    shared = open(os.path.join(CSRC, "reads_call.hip")).read()
    assert len(re.findall(r"\nint reads_require_plain\(", shared)) == 1 and shared.count("reads_plain(") == 1   # the Dna look: one owner, called here
    fastq = open(os.path.join(CSRC, "fastq_reads.hip")).read()
    assert len(re.findall(r"__global__[^;{]*\bfastq_copy_kernel\(", fastq)) == 1          # one copy kernel, for both lines
    assert len(re.findall(r"__global__[^;{]*\bfastq_rec_(?:sum|top|write)_kernel\(", fastq)) == 3   # one scan, two sources
    assert "struct LineSource" in fastq and "struct MergedSource" in fastq and "mrg_length(" in fastq
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"merge_pairs.hip"' in build and '"merge_step.h"' in build


# ---------------------------------------------------------------- the surface
def test_symbols_are_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    L = sassy.lib()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    for name in (NAME, "sassy_hip_reads_quality"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
    assert re.search(r"#define SASSY_HIP_KEEP_QUALITY\s+32u\b", hdr) and sassy.KEEP_QUALITY == 32 and "KEEP_QUALITY: u32 = 32" in rust
    assert getattr(L, NAME).restype is not None and len(getattr(L, NAME).argtypes) == 9
    assert len(L.sassy_hip_reads_quality.argtypes) == 1 and L.sassy_hip_reads_quality(None) is None
    # the flag's bit is no other flag's
    assert len({sassy.ALL_MINIMA, sassy.WITHOUT_TRACE, sassy.TEXT_ON_DEVICE, sassy.TEXT_UNCHANGED, sassy.LINE_SPANS, sassy.KEEP_QUALITY}) == 6
    assert hasattr(sassy.Searcher, "merge_pairs") and hasattr(sassy, "reads_to_fastq") and hasattr(sassy.DeviceReads, "download_quality_text")
    doc = hdr[hdr.index("/* Paired-end merge"):hdr.index("int " + NAME)]
    for word in ("min(126, 33 + max(2, |qa - qb|))", "a's on a tie", "ONE RECORD PER PAIR", "text_bytes == 64", "SASSY_HIP_KEEP_QUALITY",
                 "sassy_hip_reads_free", "qual_start = seq_start"):
        assert word in doc, word
    import inspect
    from sassy_amd import fastx
    assert "keep_quality" in inspect.signature(fastx.read_fastq_pair_device_batches).parameters
    assert "keep_quality" in inspect.signature(sassy.DeviceReads.__init__).parameters


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal the C call can raise without a read batch, with its code and a message that names the reason, in a child
    that sees no device.  The refusals that read a batch -- record counts, device, the length limit, the kept qualities -- are
    the same function's next lines: the driver above walks them, the GPU tests raise them."""
    code = r'''
import ctypes as C, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
FAKE = 0x7000000   # a batch pointer that is never read: every refusal below comes before the batches are looked at
def call(s, r1=FAKE, r2=FAKE, min_overlap=10, k=512, permille=200, flags=0, s_null=False):
    out = C.c_void_p(7)
    rc = L.sassy_hip_merge_pairs(None if s_null else s._h, r1, r2, min_overlap, k, permille, flags, None, C.byref(out))
    return rc, L.sassy_hip_last_error().decode(), out.value
def refused(s, want, word, **kw):
    rc, msg, out = call(s, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg and out is None, (rc, msg, want, word, out)
dna, iupac = sassy_amd.Searcher("dna", rc=False), sassy_amd.Searcher("iupac", rc=True)
refused(dna, EINVAL, "merge_pairs() must not be null", s_null=True)
for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.TEXT_ON_DEVICE, sassy_amd.KEEP_QUALITY, 1 << 20):
    refused(dna, EINVAL, "merge_pairs takes no flags", flags=flags)
refused(dna, EINVAL, "min_overlap must be at least 1", min_overlap=0)
refused(iupac, EINVAL, "max_permille must be <= 1000 (got 1001)", permille=1001)
for alphabet in ("ascii", "ascii_ci"):
    refused(sassy_amd.Searcher(alphabet, rc=False), EINVAL, "have no complement")
refused(sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang")
refused(sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match")
refused(sassy_amd.Searcher("dna", rc=False).with_max_n_frac(0.2), EUNSUPPORTED, "merge_pairs does not take max_n_frac")
refused(dna, EINVAL, "merge_pairs() must not be null", r1=None)
refused(dna, EINVAL, "merge_pairs() must not be null", r2=None)
# the parse: the new flag is taken, the others are refused as before; nothing without a device
res = C.c_void_p(7)
rc = L.sassy_hip_fastq_parse(b"@a\nAC\n+\nII\n", 11, sassy_amd.KEEP_QUALITY, None, C.byref(res))
assert rc == ENODEVICE and res.value is None, (rc, L.sassy_hip_last_error())
rc = L.sassy_hip_fastq_parse(b"@a\nAC\n+\nII\n", 11, sassy_amd.KEEP_QUALITY | sassy_amd.LINE_SPANS, None, C.byref(res))
assert rc == EINVAL and "SASSY_HIP_KEEP_QUALITY" in L.sassy_hip_last_error().decode()
# the Python call: lists of (sequence, quality) go through from_sequences, which refuses before anything else and then needs the device
for args, word in ((([(b"AC\nGT", b"IIIII")], [(b"ACGT", b"IIII")]), "sequence 0 holds a line end"),
                   (([(b"ACGT", b"III")], [(b"ACGT", b"IIII")]), "quality 0 has 3 bytes, its sequence 4"),
                   (([(b"ACGT", b"IIII")], [(b"ACGT", b"II\rI")]), "quality 0 holds a line end"),
                   (([(b"ACGT", b"IIII")], [(b"ACGT", b"IIII")]), "no usable HIP device"), (([], []), "no usable HIP device")):
    try:
        dna.merge_pairs(*args)
    except sassy_amd.SassyHipError as e:
        assert word in str(e), (word, e)
    else:
        raise SystemExit(3)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_from_sequences_with_qualities_parses_back(sassy):
    seqs = [b"ACGT", b"", b"NNU-x", "acgt"]
    quals = [b"IIII", b"", b"@+!~J", "5555"]
    raw = sassy.fastq_from_sequences(seqs, quals)
    assert raw == b"@\nACGT\n+\nIIII\n@\n\n+\n\n@\nNNU-x\n+\n@+!~J\n@\nacgt\n+\n5555\n"
    assert fastq_ref.records(raw) == [("", b"ACGT", b"IIII"), ("", b"", b""), ("", b"NNU-x", b"@+!~J"), ("", b"acgt", b"5555")]
    assert sassy.fastq_from_sequences(seqs) == sassy.fastq_from_sequences(seqs, None) == b"@\nACGT\n+\n\n@\n\n+\n\n@\nNNU-x\n+\n\n@\nacgt\n+\n\n"
    assert sassy.fastq_from_sequences([], []) == b""
    for bad_s, bad_q, word in (([b"ACGT"], [b"III"], "quality 0 has 3 bytes"), ([b"ACGT"], [b"II\nI"], "line end"), ([b"ACGT"], [], "1 sequences and 0 qualities"),
                               ([b"AC\rT"], [b"IIII"], "sequence 0 holds a line end")):
        with pytest.raises(sassy.SassyHipError, match=word):
            sassy.fastq_from_sequences(bad_s, bad_q)


class _FakeReads:
    """What reads_to_fastq asks of a DeviceReads, on the host."""

    def __init__(self, seqs, quals):
        self.seq_starts, self.seq_lens, self._text = mref.layout_of(seqs)
        self._qual = mref.layout_of(quals)[2]

    def __len__(self):
        return len(self.seq_lens)

    def download_text(self):
        return self._text.tobytes()

    def download_quality_text(self):
        return self._qual.tobytes()


def test_reads_to_fastq_slices_two_buffers_and_skips_empty_records(sassy):
    seqs = [b"ACGT", b"", b"G" * 64, b"T" * 65, b"", b"A"]
    quals = [b"IJKL", b"", b"#" * 64, b"5" * 64 + b"6", b"", b"~"]
    ids = ["r0 x", "r1", b"r2", "", "r4", "r5/1"]
    got = sassy.reads_to_fastq(_FakeReads(seqs, quals), ids)
    want = b"".join(b"@" + (i.encode() if isinstance(i, str) else i) + b"\n" + s + b"\n+\n" + q + b"\n" for i, s, q in zip(ids, seqs, quals) if s)
    assert got == want
    assert [(i, s, q) for i, s, q in fastq_ref.records(got)] == [("r0 x", seqs[0], quals[0]), ("r2", seqs[2], quals[2]), ("", seqs[3], quals[3]),
                                                                ("r5/1", seqs[5], quals[5])]
    assert sassy.reads_to_fastq(_FakeReads([b"", b""], [b"", b""]), ["a", "b"]) == b"" and sassy.reads_to_fastq(_FakeReads([], []), []) == b""
    with pytest.raises(sassy.SassyHipError, match="2 reads and 1 ids"):
        sassy.reads_to_fastq(_FakeReads([b"A", b"C"], [b"I", b"I"]), ["a"])


# ---------------------------------------------------------------- CLI
def test_cli_merge_parser(sassy, capsys):
    from sassy_amd import cli
    import argparse
    ap = argparse.ArgumentParser()
    mp = cli.merge_parser(ap.add_subparsers(dest="cmd"))
    args = mp.parse_args(["a.fq", "b.fq"])
    assert (args.r1, args.r2, args.output, args.unmerged1, args.unmerged2, args.min_overlap, args.k, args.max_permille, args.alphabet, args.tsv) == \
        ("a.fq", "b.fq", "", "", "", 10, 512, 200, "dna", False)
    args = mp.parse_args(["a.fq", "b.fq", "-o", "m.fq", "--unmerged1", "u1.fq", "--unmerged2", "u2.fq", "--min-overlap", "4", "-k", "1", "--max-permille", "0",
                          "--alphabet", "iupac", "--tsv"])
    assert (args.output, args.unmerged1, args.unmerged2, args.min_overlap, args.k, args.max_permille, args.alphabet, args.tsv) == \
        ("m.fq", "u1.fq", "u2.fq", 4, 1, 0, "iupac", True)
    with pytest.raises(SystemExit):
        mp.parse_args(["a.fq", "b.fq", "--alphabet", "ascii"])
    capsys.readouterr()
    for argv in (["--min-overlap", "0"], ["--max-permille", "1001"], ["-k", "-1"]):
        with pytest.raises(SystemExit):
            cli.main(["merge", "a.fq", "b.fq"] + argv)
        assert "merge takes --min-overlap >= 1" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["merge", "a.fq", "b.fq", "--tsv"])
    assert "needs -o" in capsys.readouterr().err
