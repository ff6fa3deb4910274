"""CPU-only: adapter and quality trimming (sassy_hip_trim_reads, Searcher.trim_reads, `trim`) and the window call
(sassy_hip_reads_slice) -- what needs no device: the definition's helper on the cases written out by hand and against a brute
force in plain Python, the quality rule against a literal transcription of its loop, the arithmetic of trim_step.h driven by a
stand-alone host program under AddressSanitizer / UBSan, the step header's and the unit's layout, the symbols, every refusal
the C call can raise without a read batch, the CLI's parser."""
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

import trim_reads_ref as tref  # noqa: E402
from hamming_ref import relation_row  # noqa: E402

NAME = "sassy_hip_trim_reads"
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


@pytest.fixture(scope="module")
def sassy():
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


# ---------------------------------------------------------------- the definition
def test_helper_reproduces_the_cases_written_out_by_hand():
    assert len(tref.HAND) == 5
    for case in tref.HAND:
        records, seqs, quals = tref.expected_trim("dna", [(case["seq"], case["qual"])], case["adapters"], **case["call"])
        assert tuple(records[0].tolist()) == case["record"], (case["name"], records)
        n = case["record"][0]
        assert (seqs[0], quals[0]) == (case["seq"][:n], case["qual"][:n]), case["name"]
    by_name = {c["name"]: c for c in tref.HAND}
    # the early stop matters: without it the walk would reach the lower stretch further left and leave nothing
    q = by_name["the early stop of the quality walk"]["qual"]
    terms = [c - 33 - 20 for c in q]
    sums = [sum(terms[i:]) for i in range(len(q))]
    assert min(sums) == sums[0] < sums[10] < 0 < sums[8] and tref.quality_len(q, 20) == 10
    # two adapters at one c: j = 1 and j = 2 tie in everything, j = 3 has the same density and a shorter overlap
    assert by_name["two adapters at one position"]["record"][3] == 1
    assert by_name["dropped by min_length"]["record"][0] == 0 and by_name["dropped by min_length"]["record"][2] == 5


def _literal_quality(q, cutoff):
    """The loop of the definition, transcribed."""
    la = len(q)
    if cutoff == 0:
        return la
    s, lowest, lq = 0, 0, la
    for i in range(la - 1, -1, -1):
        s += q[i] - 33 - cutoff
        if s > 0:
            break
        if s < lowest:
            lowest, lq = s, i
    return lq


def _brute(profile, seq, qual, adapters, min_overlap, k, max_permille, quality_cutoff, min_length):
    """The definition position by position in plain Python (no numpy)."""
    lq = _literal_quality(qual, quality_cutoff)
    best = None
    for c in range(lq):
        for j, ad in enumerate(adapters):
            ov = min(len(ad), lq - c)
            mm = sum(1 for i in range(ov) if not relation_row(profile, ad[i])[seq[c + i]])
            if ov >= min_overlap and mm <= k and mm * 1000 <= max_permille * ov:
                if best is None or mm * best[2] < best[1] * ov or (mm * best[2] == best[1] * ov and ov > best[2]):
                    best = (c, mm, ov, j)
        if best:
            break
    cut = best[0] if best else lq
    return (cut if cut >= min_length else 0, lq, cut, best[3] if best else -1, best[2] if best else 0, best[1] if best else 0)


def test_helper_against_a_brute_force_on_random_reads():
    rnd = random.Random(5)
    letters = {"dna": b"ACGT", "iupac": b"ACGTNUNRYacgtn-X"}
    for profile in ("dna", "iupac"):
        found = dropped = 0
        for _ in range(300):
            la = rnd.randrange(40)
            adapters = [bytes(rnd.choice(letters[profile]) for _ in range(rnd.choice((3, 5, 8, 13)))) for _ in range(rnd.randrange(1, 4))]
            seq = bytearray(rnd.choice(letters[profile]) for _ in range(la))
            if la and rnd.random() < 0.8:
                ad, c = rnd.choice(adapters), rnd.randrange(la)
                seq[c:] = (ad + bytes(seq[c:]))[:la - c]
            qual = bytes(rnd.randrange(33, 75) for _ in range(la))
            call = dict(min_overlap=rnd.randrange(1, 4), k=rnd.choice((0, 1, 2, 512)), max_permille=rnd.choice((0, 100, 250, 1000)),
                        quality_cutoff=rnd.choice((0, 0, 10, 25)), min_length=rnd.choice((0, 0, 5, 20)))
            rec = tref.trim_one(profile, bytes(seq), qual, adapters, **call)
            assert rec == _brute(profile, bytes(seq), qual, adapters, **call), (profile, bytes(seq), adapters, call)
            found += rec[3] >= 0
            dropped += rec[0] == 0 and rec[2] > 0
        assert found > 100 and dropped > 0, (profile, found, dropped)


def test_quality_rule_against_the_loop_of_the_definition():
    rnd = random.Random(9)
    cases = [(b"", 20), (b"!" * 30, 20), (b"~" * 30, 20), (b"5" * 30, 20), (b"5", 20), (b"I" * 10 + b"#" * 5, 20), (b"#" * 5 + b"I" * 10, 20),
             (b"#5#5#5#5", 20), (b"5555#55#", 20), (b"IIII", 0), (b"#" * 200, 93), (b"~" * 200, 93)]
    for _ in range(400):
        la = rnd.randrange(0, 80)
        centre = rnd.choice((35, 53, 73))
        cases.append((bytes(min(126, max(33, centre + rnd.randrange(-4, 5))) for _ in range(la)), rnd.choice((1, 2, 20, 40, 93))))
    for q, cutoff in cases:
        assert tref.quality_len(q, cutoff) == _literal_quality(q, cutoff), (q, cutoff)
    assert tref.quality_len(b"!" * 30, 20) == 0 and tref.quality_len(b"~" * 30, 20) == 30 and tref.quality_len(b"5" * 30, 20) == 30  # all low, all high, all ties
    assert tref.quality_len(b"", 20) == 0 and tref.quality_len(b"5555#55#", 20) == 4  # ('5' is Phred 20: a tie keeps the larger index)


# ---------------------------------------------------------------- the step header
LENGTHS = list(range(131)) + [191, 192, 193, 255, 256, 257, 511, 512]
ADAPTER_LENS = (1, 31, 32, 33, 63, 64)


def test_step_arithmetic_against_a_byte_wise_brute_force_under_sanitizers(tmp_path):
    """tests/c/trim_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: trim_step.h as the kernels call it, 64 lanes simulated, against a byte-wise brute force."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "trim_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "c", "trim_step_driver.cc")])
    r = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    fields = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}
    # per profile, read length, adapter length and word count (the kernel's and the widest): once unplanted, once per position
    assert fields["reads"] == 2 * len(LENGTHS) * len(ADAPTER_LENS) * 2, fields
    assert fields["positions"] == 2 * sum(LENGTHS) * len(ADAPTER_LENS) * 2, fields
    assert fields["walks"] == 7 * 2 * len(LENGTHS), fields   # seven kinds of qualities per length and word count
    assert fields["refusals"] == 25, fields                  # 20 refusals, the adapters' null twice and the handle's judged late, 3 x ok
    # the windows: 34 begins, two tails, two starts, and per length its blocks
    assert fields["blocks"] == 34 * 2 * 2 * sum((n + 63) // 64 for n in (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)), fields


def test_step_header_is_free_of_hip_and_the_driver_stands_alone():
    src = open(os.path.join(CSRC, "trim_step.h")).read()
    code = re.sub(r"//.*", "", src)
    assert "#include <hip" not in src and "hipStream" not in src and "getenv" not in src
    assert "__builtin_amdgcn" not in src and "__HIP_DEVICE_COMPILE__" not in src and "asm" not in code and "switch" not in code
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>", '#include "fastq_step.h"',
                                                                         '#include "overlap_step.h"']
    for fn in ("trm_refusal", "trm_term", "trm_scan_add", "trm_stop_lane", "trm_low_combine", "trm_window", "trm_mismatches", "trm_better", "trm_combine",
               "trm_record", "trm_window_block"):
        assert re.search(r"\b" + fn + r"\s*\(", src), fn
    # the acceptance rule is overlap_step.h's: not restated here
    assert "* 1000u" not in code and "ovl_accepts" not in code
    assert "ovl_mismatch_word<P, IUPAC>(" in code and "fq_shift_block(" in code and "pairs_row_code(" in code
    # the order and the combine are branch-free
    body = src[src.index("SASSY_HAM_HD bool trm_better("):src.index("SASSY_HAM_HD TrmBest trm_one(")]
    assert "if (" not in body and "&&" not in re.sub(r"//.*", "", body) and "||" not in re.sub(r"//.*", "", body)
    driver = open(os.path.join(ROOT, "tests", "c", "trim_step_driver.cc")).read()
    assert "int main(" in driver and "#include <hip" not in driver and "__global__" not in driver and "trim_step.h" in driver


def test_source_layout():
    """The entry points live in trim_reads.hip with two kernels, no inline assembly, no atomics, no switch and no environment;
    the acceptance is overlap_step.h's; the scan is fastq_reads.hip's with further sources of lengths."""
    unit = open(os.path.join(CSRC, "trim_reads.hip")).read()
    code = re.sub(r"//.*", "", unit)
    assert "int " + NAME + "(" in unit and "int sassy_hip_reads_slice(" in unit
    assert "asm" not in code and "getenv" not in code and "atomic" not in code and "switch" not in code
    assert len(re.findall(r"__global__[^;{]*\btrim_find_kernel\(", unit)) == 1 and len(re.findall(r"__global__[^;{]*\breads_window_write_kernel\(", unit)) == 1
    assert code.count("__global__") == 2
    assert "ovl_accepts(" in code and "trm_refusal(" in code and "trm_combine(" in code and "trm_window_block(" in code
    assert "reads_layout_trimmed(" in code and "windows_from_host(" in code and "reads_require_plain(" in code
    shared = open(os.path.join(CSRC, "reads_call.hip")).read()
    assert len(re.findall(r"\nint reads_require_plain\(", shared)) == 1 and shared.count("reads_plain(") == 1   # the Dna look: one owner, called here
    assert len(re.findall(r"\nint windows_from_host\(", shared)) == 1 and shared.count("reads_layout_windows(") == 1   # the slice's layout: likewise
    assert "ham_text_of(" in code and "ham_rem(" in code and "hipMemset(" not in code
    assert "fastq_rec_" not in code                                    # no scan of its own
    host = open(os.path.join(CSRC, "host_internal.h")).read()
    for decl in ("int reads_layout_trimmed(", "int reads_layout_windows("):
        assert decl in host, decl
    fastq = open(os.path.join(CSRC, "fastq_reads.hip")).read()
    assert len(re.findall(r"__global__[^;{]*\bfastq_rec_(?:sum|top|write)_kernel\(", fastq)) == 3   # one scan, four sources
    for src in ("struct LineSource", "struct MergedSource", "struct TrimSource", "struct WindowSource"):
        assert src in fastq, src
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"trim_reads.hip"' in build and '"trim_step.h"' in build


# ---------------------------------------------------------------- the surface
def test_symbols_are_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    L = sassy.lib()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    for name in (NAME, "sassy_hip_reads_slice"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
    assert re.search(r"#define SASSY_HIP_TRIM_MAX_ADAPTERS\s+64u\b", hdr) and sassy.TRIM_MAX_ADAPTERS == 64 and "TRIM_MAX_ADAPTERS: u32 = 64" in rust
    assert len(getattr(L, NAME).argtypes) == 13 and len(L.sassy_hip_reads_slice.argtypes) == 5
    assert sassy.read_trim_dtype() == tref.DTYPE and sassy.read_trim_dtype().itemsize == 16
    assert hasattr(sassy.Searcher, "trim_reads") and hasattr(sassy.DeviceReads, "slice")
    doc = hdr[hdr.index("/* Adapter and quality trimming"):hdr.index("int " + NAME)]
    for word in ("ONE RECORD PER READ", "text_bytes == 64", "SASSY_HIP_KEEP_QUALITY", "sassy_hip_reads_free", "qual_start = seq_start",
                 "mm * 1000 <= max_permille * ov", "the smallest c", "quality_cutoff > 93", "scan_launches = 5, or 6"):
        assert word in doc, word
    import inspect
    from sassy_amd import fastx
    assert "keep_quality" in inspect.signature(fastx.read_fastq_device_batches).parameters
    sig = inspect.signature(sassy.Searcher.trim_reads).parameters
    assert [(k, v.default) for k, v in list(sig.items())[3:]] == [("min_overlap", 3), ("k", 512), ("max_permille", 100), ("quality_cutoff", 0),
                                                                  ("min_length", 0), ("with_records", False)]


def test_every_inherited_public_method_has_an_entry_of_the_extension(sassy):
    """tests/test_call_catalogue_cpu.py keeps every public method of Searcher itself in the call catalogue; the methods Searcher
    inherits are kept here in the catalogue's extension (tests/helpers/call_catalogue_ext.py), which
    tests/test_gpu_trim_call_order.py walks against every entry of the catalogue.  A method added to a base class of Searcher
    fails here until it has an entry."""
    import inspect
    import call_catalogue as cc
    import call_catalogue_ext as ext
    exempt = ("set_", "with_", "get_", "enable_", "_")
    inherited = [name for base in sassy.Searcher.__mro__[1:] if base is not object
                 for name, f in vars(base).items() if inspect.isfunction(f) and not name.startswith(exempt)]
    assert inherited == ["trim_reads"], inherited
    named = {m for e in ext.ENTRIES for m in e.methods}
    assert named == set(inherited) and all(hasattr(sassy.Searcher, m) for m in named)
    # per kind that can run it a real call, per kind that cannot a refusal; every entry names a kind and is no catalogue entry
    assert {k for e in ext.ENTRIES if not e.refusal for k in e.kinds} == set(cc.NUC)
    assert {k for e in ext.ENTRIES if e.refusal for k in e.kinds} == set(cc.PLAIN)
    assert len(cc.ENTRIES) == 82 and not {e.name for e in ext.ENTRIES} & {e.name for e in cc.ENTRIES}   # the catalogue is only read
    for kind in cc.NUC:
        want = ext.expected(kind, "trim_reads")
        hash(want)
        assert ext.ENTRIES[0].size_of(want) >= 3, (kind, "expects no adapter found")


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal the C call can raise without a read batch, with its code and a message that names the reason, in their
    order, in a child that sees no device.  The refusals that read the batch are the same function's next lines: the driver
    above walks them, the GPU tests raise them."""
    code = r'''
import ctypes as C, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
FAKE = 0x7000000   # a batch pointer that is never read: every refusal below comes before the batch is looked at
def call(s, adapters=(b"ACGTAC",), reads=FAKE, min_overlap=3, k=512, permille=100, cutoff=0, min_length=0, flags=0, s_null=False, null_at=None, lens=None,
         arrays=True):
    n = len(adapters)
    ptrs = (C.c_char_p * max(n, 1))(*[None if i == null_at else a for i, a in enumerate(adapters)])
    ls = (C.c_size_t * max(n, 1))(*(lens or [len(a) for a in adapters]))
    out = C.c_void_p(7)
    rc = L.sassy_hip_trim_reads(None if s_null else s._h, reads, ptrs if arrays else None, ls if arrays else None, n, min_overlap, k, permille, cutoff,
                                min_length, flags, None, C.byref(out))
    return rc, L.sassy_hip_last_error().decode(), out.value
def refused(s, want, word, **kw):
    rc, msg, out = call(s, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg and out is None, (rc, msg, want, word, out)
dna, iupac = sassy_amd.Searcher("dna", rc=False), sassy_amd.Searcher("iupac", rc=True)
everything = dict(flags=1, min_overlap=0, permille=1001, cutoff=94, adapters=(b"A",) * 65, reads=None)   # each refusal hides the ones behind it
refused(dna, EINVAL, "trim_reads() must not be null", s_null=True, **everything)
refused(dna, EINVAL, "trim_reads takes no flags", **everything)
for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.TEXT_ON_DEVICE, sassy_amd.KEEP_QUALITY, 1 << 20):
    refused(dna, EINVAL, "trim_reads takes no flags", flags=flags)
everything.pop("flags")
refused(dna, EINVAL, "min_overlap must be at least 1", **everything)
everything["min_overlap"] = 2
refused(iupac, EINVAL, "max_permille must be <= 1000 (got 1001)", **everything)
everything.pop("permille")
refused(dna, EINVAL, "quality_cutoff must be <= 93 (Phred+33; got 94)", **everything)
everything.pop("cutoff")
refused(dna, EINVAL, "at most 64 adapters (SASSY_HIP_TRIM_MAX_ADAPTERS; got 65)", **everything)
ascii_ = sassy_amd.Searcher("ascii", rc=False)
refused(ascii_, EINVAL, "must not be null (adapter 0)", arrays=False, reads=None)
refused(ascii_, EINVAL, "must not be null (adapter 1)", adapters=(b"ACGT", b"ACGT"), null_at=1, reads=None)
refused(ascii_, EINVAL, "adapter 1 is empty", adapters=(b"ACGT", b"ACGT"), lens=[4, 0], reads=None)
refused(ascii_, EINVAL, "adapter 0 has 65 bytes: an adapter has at most 64", adapters=(b"A" * 65,), reads=None)
refused(ascii_, EINVAL, "adapter 2 has 3 bytes, fewer than min_overlap = 4", adapters=(b"ACGT", b"ACGTA", b"ACG"), min_overlap=4, reads=None)
for alphabet in ("ascii", "ascii_ci"):
    refused(sassy_amd.Searcher(alphabet, rc=False), EINVAL, "use a dna or an iupac searcher", reads=None)
refused(sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang", reads=None)
refused(sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match", reads=None)
refused(sassy_amd.Searcher("dna", rc=False).with_max_n_frac(0.2), EUNSUPPORTED, "trim_reads does not take max_n_frac", reads=None)
refused(dna, EINVAL, "trim_reads() must not be null", reads=None)
refused(dna, EINVAL, "trim_reads() must not be null", reads=None, adapters=())
# the slice: its pointers
out = C.c_void_p(7)
assert L.sassy_hip_reads_slice(None, None, None, None, C.byref(out)) == EINVAL and out.value is None and "reads_slice() must not be null" in L.sassy_hip_last_error().decode()
# the Python call: lists go through from_sequences, which refuses before anything else and then needs the device
for args, word in ((([(b"AC\nGT", b"IIIII")], [b"ACGT"]), "sequence 0 holds a line end"), (([(b"ACGT", b"III")], [b"ACGT"]), "quality 0 has 3 bytes, its sequence 4"),
                   (([b"ACGT"], [b"ACGT"]), "no usable HIP device"), (([], []), "no usable HIP device")):
    try:
        dna.trim_reads(*args)
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
def test_cli_trim_parser(sassy, capsys):
    from sassy_amd import cli
    import argparse
    ap = argparse.ArgumentParser()
    tp = cli.trim_parser(ap.add_subparsers(dest="cmd"))
    args = tp.parse_args(["in.fq"])
    assert (args.input, args.adapter, args.output, args.quality_cutoff, args.min_length, args.min_overlap, args.k, args.max_permille, args.alphabet, args.tsv) == \
        ("in.fq", [], "", 0, 0, 3, 512, 100, "dna", False)
    args = tp.parse_args(["in.fq", "-a", "AGATCGGAAGAGC", "-a", "CTGTCTCTTATA", "-o", "t.fq", "-q", "20", "-m", "30", "--min-overlap", "5", "-k", "2",
                          "--max-permille", "0", "--alphabet", "iupac", "--tsv"])
    assert (args.adapter, args.output, args.quality_cutoff, args.min_length, args.min_overlap, args.k, args.max_permille, args.alphabet, args.tsv) == \
        (["AGATCGGAAGAGC", "CTGTCTCTTATA"], "t.fq", 20, 30, 5, 2, 0, "iupac", True)
    with pytest.raises(SystemExit):
        tp.parse_args(["in.fq", "--alphabet", "ascii"])
    capsys.readouterr()
    for argv in (["--min-overlap", "0"], ["--max-permille", "1001"], ["-k", "-1"], ["-q", "94"], ["-m", "-1"]):
        with pytest.raises(SystemExit):
            cli.main(["trim", "in.fq"] + argv)
        assert "trim takes --min-overlap >= 1" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["trim", "in.fq", "-a", "A" * 65])
    assert "up to 64 adapters of 1 .. 64 bases" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["trim", "in.fq", "--tsv"])
    assert "needs -o" in capsys.readouterr().err
    records = np.array([(10, 28, 10, 0, 13, 0), (0, 5, 5, -1, 0, 0)], dtype=tref.DTYPE)
    assert cli.trim_rows(["r0 x", "r1"], records) == ["r0 x\t10\t28\t10\t0\t13\t0\n", "r1\t0\t5\t5\t-1\t0\t0\n"]
    assert cli.TRIM_HEADER.count("\t") == 6
