"""FASTQ parse on the device and the Hamming batch calls over its read batch (sassy_hip_fastq_parse, sassy_hip_*_reads,
sassy_amd.DeviceReads): everything that needs no device -- the definition against the host reader, the bit arithmetic under
sanitizers, the symbols, every refusal that comes before device work, the loud failure without a device, the CLI flag, the
strings other tests count in the Hamming sources.  The kernels themselves: tests/test_gpu_fastq_reads.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import fastq_ref  # noqa: E402

PARSE_NAMES = ("sassy_hip_fastq_parse", "sassy_hip_reads_n", "sassy_hip_reads_records", "sassy_hip_reads_text", "sassy_hip_reads_text_bytes",
               "sassy_hip_reads_longest", "sassy_hip_reads_rem", "sassy_hip_reads_free")
CALL_NAMES = ("sassy_hip_search_hamming_reads", "sassy_hip_hamming_best_pattern_reads", "sassy_hip_hamming_counts_reads")


@pytest.fixture(scope="module")
def sassy():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


def test_definition_equals_the_host_reader(tmp_path):
    from sassy_amd.fastx import read_fastx_batches
    for name, data in fastq_ref.corpus().items():
        (tmp_path / name).write_bytes(data)
        want = fastq_ref.records(data)
        for bb in (64, 1000, 1 << 20):
            got = []
            for rb in read_fastx_batches(str(tmp_path / name), bb):
                got += [(rb.id(i), rb.sequence(i), rb.quality(i)) for i in range(len(rb))]
            assert got == want, (name, bb, got[:3], want[:3])
        # the numpy form of the definition, which the GPU tests use for inputs of millions of records
        reads = fastq_ref.parse(data)
        cols, src = fastq_ref.columns(data)
        table = fastq_ref.table(reads)
        assert all(np.array_equal(cols[c], table[c]) for c in table), name
        assert fastq_ref.layout_np(data, cols, src).tobytes() == fastq_ref.layout(reads), name


def test_both_sides_refuse_malformed_input(tmp_path):
    from sassy_amd.fastx import read_fastx_batches
    for name, (data, record, rule) in fastq_ref.malformed().items():
        for parse in (fastq_ref.parse, fastq_ref.columns):
            with pytest.raises(fastq_ref.Malformed) as e:
                parse(data)
            assert (e.value.record, e.value.rule) == (record, rule), (name, str(e.value))
        (tmp_path / name).write_bytes(data)
        for bb in (64, 1000, 1 << 20):
            with pytest.raises(ValueError):
                for rb in read_fastx_batches(str(tmp_path / name), bb):
                    pass


def test_definition_on_a_case_written_out_by_hand():
    raw = b"@r1 d\r\nAC\rG\r\n+r1\r\n!!!!\n@\n\n+\n\n@r3\nACGT\n+\n@III"
    #       0        7        13     19      24 26 27 28 30    34    39 41
    reads = fastq_ref.parse(raw)
    assert [(raw[r.id_start:r.id_start + r.id_len], r.seq, r.seq_start, raw[r.qual_start:r.qual_start + r.qual_len]) for r in reads] == \
        [(b"r1 d", b"AC\rG", 0, b"!!!!"), (b"", b"", 64, b""), (b"r3", b"ACGT", 64, b"@III")]
    assert [(r.id_start, r.id_len, r.qual_start, r.qual_len) for r in reads] == [(1, 4, 18, 4), (24, 0, 28, 0), (30, 2, 40, 4)]
    text = fastq_ref.layout(reads)
    assert len(text) == 128 + 64 and text[:4] == b"AC\rG" and text[64:68] == b"ACGT" and not any(text[4:64]) and not any(text[68:])
    assert fastq_ref.parse(b"") == [] and fastq_ref.layout([]) == bytes(64)
    assert fastq_ref.rem([0, 64, 64, 256, 256], [4, 0, 130, 0, 0]).tolist() == [4, 130, 66, 2]


def test_symbols_are_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    for name in PARSE_NAMES + CALL_NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(sassy.lib(), name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
    assert "} sassy_hip_ReadRecord;" in hdr and "pub struct ReadRecord" in rust and sassy.read_record_dtype().itemsize == 48
    L = sassy.lib()
    assert len(L.sassy_hip_fastq_parse.argtypes) == 5
    assert all(len(getattr(L, n).argtypes) == 1 for n in PARSE_NAMES[1:])
    # a handle where the _many sibling takes texts, text_lens, n_texts
    for name, many in zip(CALL_NAMES, ("sassy_hip_search_hamming_many", "sassy_hip_hamming_best_pattern", "sassy_hip_hamming_counts_many")):
        assert len(getattr(L, name).argtypes) == len(getattr(L, many).argtypes) - 2, name
    assert hasattr(sassy, "DeviceReads")
    from sassy_amd import fastx
    assert hasattr(fastx, "read_fastq_device_batches") and hasattr(fastx, "read_fasta_device_batches")
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"fastq_reads.hip"' in build and '"fastq_step.h"' in build


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal with its code and a message that names the reason, in a child that sees no device: a call that got as far
    as the device would say 'no usable HIP device' instead.  Then valid arguments: that message, loudly, from the C call, from
    DeviceReads and from the reader."""
    code = r'''
import ctypes as C, os, sys, tempfile, sassy_amd
from sassy_amd import fastx
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
def call(raw, n=None, flags=0, out=True, addr=None):
    res = C.c_void_p(7)
    n = len(raw) if n is None else n
    rc = L.sassy_hip_fastq_parse(addr if addr is not None else raw, n, flags, None, C.byref(res) if out else None)
    return rc, L.sassy_hip_last_error().decode(), res.value
def refused(want, word, *a, **kw):
    rc, msg, res = call(*a, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (rc, msg, want, word)
    if kw.get("out", True):
        assert res is None, res  # nothing comes back
ok = b"@a\nACGT\n+\nIIII\n"
refused(EINVAL, "null argument", None, n=8)
refused(EINVAL, "null argument", ok, out=False)
refused(EINVAL, "first byte is not '@'", b"ACGT\n")
refused(EINVAL, "first byte is not '@'", b"\n@a\nAC\n+\nII\n")
refused(EINVAL, "first byte is not '@'", b">a\nAC\n")
for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.ALL_MINIMA, sassy_amd.TEXT_UNCHANGED, sassy_amd.LINE_SPANS, 1 << 20,
              sassy_amd.TEXT_ON_DEVICE | sassy_amd.TEXT_UNCHANGED):
    refused(EINVAL, "fastq_parse takes SASSY_HIP_TEXT_ON_DEVICE only", ok, flags=flags)
for addr in (0x7000001, 0x7000008, 0x700000f):
    refused(EINVAL, "16-byte aligned", None, n=8, flags=sassy_amd.TEXT_ON_DEVICE, addr=addr)
refused(EUNSUPPORTED, "too long for the tile index", ok, n=1 << 47)  # (refused on its length: byte 0 is all that is read)
refused(EUNSUPPORTED, "too long for the tile index", None, n=(1 << 47) - 65535, flags=sassy_amd.TEXT_ON_DEVICE, addr=0x7000000)
assert L.sassy_hip_reads_n(None) == 0 and L.sassy_hip_reads_records(None) is None and L.sassy_hip_reads_rem(None) is None
assert L.sassy_hip_reads_text(None) is None and L.sassy_hip_reads_text_bytes(None) == 0 and L.sassy_hip_reads_longest(None) == 0
L.sassy_hip_reads_free(None)
# valid arguments get as far as the device, and fail loudly there
for raw, kw in ((ok, {}), (b"", {}), (b"@", {}), (None, dict(n=0)), (None, dict(n=(1 << 47) - 65536, flags=sassy_amd.TEXT_ON_DEVICE, addr=0x7000000))):
    rc, msg, res = call(raw, **kw)
    assert rc == ENODEVICE and "no usable HIP device" in msg and res is None, (rc, msg, res)
try:
    sassy_amd.DeviceReads(ok)
except sassy_amd.SassyHipError as e:
    assert "no usable HIP device" in str(e), e
else:
    raise SystemExit(3)
d = tempfile.mkdtemp()
fa, fq = os.path.join(d, "a.fa"), os.path.join(d, "a.fq")
open(fa, "wb").write(b">a\nACGT\n"); open(fq, "wb").write(ok)
try:
    list(fastx.read_fastq_device_batches(fq))
except sassy_amd.SassyHipError as e:
    assert "no usable HIP device" in str(e), e
else:
    raise SystemExit(4)
try:
    list(fastx.read_fastq_device_batches(fa))
except ValueError as e:
    assert "FASTQ" in str(e), e
else:
    raise SystemExit(5)
# the batch calls: a null handle, before anything else
s = sassy_amd.Searcher("dna", rc=True)
pp, pl = (C.c_char_p * 1)(b"ACGT"), (C.c_size_t * 1)(4)
out = C.c_void_p(7)
rc = L.sassy_hip_search_hamming_reads(s._h, pp, pl, 1, None, 1, 0, C.byref(out))
assert rc == EINVAL and "search_hamming_reads() must not be null" in L.sassy_hip_last_error().decode() and out.value is None
cost = (C.c_uint8 * 4)()
rc = L.sassy_hip_hamming_best_pattern_reads(s._h, pp, pl, 1, None, 1, 0, cost, None, None, None)
assert rc == EINVAL and "hamming_best_pattern_reads() must not be null" in L.sassy_hip_last_error().decode()
counts = (C.c_uint64 * 4)()
rc = L.sassy_hip_hamming_counts_reads(s._h, pp, pl, 1, None, 1, 0, counts)
assert rc == EINVAL and "hamming_counts_reads() must not be null" in L.sassy_hip_last_error().decode()
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_step_arithmetic_against_a_byte_wise_parse_under_sanitizers(tmp_path):
    """tests/c/fastq_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: every lane shape and random lanes at every length and carried class against the byte-wise
    definition, whole inputs through the two-level count and the line pass, the layout scan and the block copy."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fastq_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "fastq_step_driver.cc")])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
        assert int(fields["lanes"]) == 2761 and int(fields["combines"]) == 124 and int(fields["layouts"]) == 1088


def test_step_header_is_free_of_hip_and_the_unit_of_assembly():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "fastq_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "__builtin_amdgcn" not in src
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>"]
    unit = open(os.path.join(ROOT, "sassy_amd", "csrc", "fastq_reads.hip")).read()
    assert '#include "fastq_step.h"' in unit and '#include "hamming_step.h"' in unit and "asm" not in re.sub(r"//.*", "", unit)
    # the block copy finds its read and its rem[] with the batch scan's own functions
    assert "ham_text_of(" in unit and "ham_rem(" in unit and "ham_rem_kernel" not in re.sub(r"//.*", "", unit)


def test_the_strings_other_tests_count_in_the_hamming_sources_still_hold():
    ham = open(os.path.join(ROOT, "sassy_amd", "csrc", "hamming.hip")).read()
    assert ham.count("hamming_refusals(s, patterns, pattern_lens, n_patterns, k,") == 3
    assert ham.count("only_best_match is not supported") == 1 and ham.count("SASSY_NO_TICKETS") == 1
    assert ham.count("int hamming_count_call(") == 1 and ham.count("return hamming_count_call(s, patterns,") == 2
    assert ham.count("\nint hamming_refusals(") == 1 and ham.count("ham_walk_ranges(S, J, P") == 1
    host = open(os.path.join(ROOT, "sassy_amd", "csrc", "host_internal.h")).read()
    assert host.count("ham_scan_range(S, J, P") == 1
    a, b = host.index("int hamming_call("), host.index("int ham_one_text(")
    assert a < b and "ensure_device()" in host[a:b]
    # the refusals stay one function: the new entry points call it, and copy none of its checks
    unit = open(os.path.join(ROOT, "sassy_amd", "csrc", "fastq_reads.hip")).read()
    assert unit.count("hamming_refusals(s, patterns, pattern_lens, n_patterns, k, who)") == 2 and "hamming_reads_counts(" in unit
    assert "only_best" not in unit and "max_overhang" not in unit and "valid_pattern" not in unit
    # no upload, no layout, no table in the batch calls
    calls = unit[unit.index("int sassy_hip_search_hamming_reads("):]
    assert "hipMemcpy" not in calls and "layout_and_upload" not in calls and "hipMalloc" not in calls


def test_cli_takes_device_parse_on_demux_and_count(sassy, capsys, monkeypatch, tmp_path):
    from sassy_amd import cli
    fq, fa, gz = tmp_path / "r.fq", tmp_path / "g.fa", tmp_path / "r.fq.gz"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    fa.write_bytes(b">g\nACGT\n")
    import gzip
    gz.write_bytes(gzip.compress(fq.read_bytes()))
    seen = {}
    monkeypatch.setattr(cli, "run_demux", lambda args, *a: seen.setdefault("demux", args) and 0)
    monkeypatch.setattr(cli, "run_count", lambda args, *a: seen.setdefault("count", args) and 0)
    monkeypatch.setattr(cli, "load_count_patterns", lambda path: [])
    for path in (fq, gz):
        seen.clear()
        cli.main(["demux", "-p", "ACGT", "-k", "1", "--device-parse", str(path)])
        cli.main(["count", "p.txt", str(path), "-k", "1", "--device-parse"])
        assert seen["demux"].device_parse and seen["count"].device_parse and not seen["count"].per_record
    seen.clear()
    cli.main(["demux", "-p", "ACGT", "-k", "1", str(fq)])
    cli.main(["count", "p.txt", str(fq), "-k", "1"])
    assert not seen["demux"].device_parse and not seen["count"].device_parse
    for argv in (["demux", "-p", "ACGT", "-k", "1", "--device-parse", str(fa)], ["count", "p.txt", str(fq), str(fa), "-k", "1", "--device-parse"],
                 ["count", "p.txt", str(fq), "-k", "1", "--device-parse", "--per-record"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert "--device-parse" in capsys.readouterr().err, argv
    for cmd in ("search", "filter"):
        with pytest.raises(SystemExit):
            cli.main([cmd, "-p", "ACGT", "-k", "1", "--device-parse", str(fq)])
        assert "--device-parse" in capsys.readouterr().err
    # --device-unwrap keeps its refusals
    with pytest.raises(SystemExit):
        cli.main(["count", "p.txt", str(fa), "-k", "1", "--device-unwrap"])
    assert "the batch call takes host texts only" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["demux", "-p", "ACGT", "-k", "1", "--device-unwrap", str(fa)])
    assert "--device-unwrap" in capsys.readouterr().err
