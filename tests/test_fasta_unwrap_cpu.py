"""FASTA unwrap on the device (sassy_hip_fasta_unwrap, sassy_amd.DeviceFasta): everything that needs no device -- the
definition against the host reader, the bit arithmetic under sanitizers, every refusal, the loud failure without a device,
the CLI flag.  The kernels themselves: tests/test_gpu_fasta_unwrap.py."""
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import fasta_ref  # noqa: E402

NAMES = ("sassy_hip_fasta_unwrap", "sassy_hip_fasta_n_records", "sassy_hip_fasta_records", "sassy_hip_fasta_text",
         "sassy_hip_fasta_text_bytes", "sassy_hip_fasta_free")


@pytest.fixture(scope="module")
def sassy():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


def corpus():
    """The FASTA files of test_fastx_batches_equal_a_line_by_line_parse (same seed, same order of draws), then the edge inputs."""
    rng = random.Random(5)
    seq = lambda n: bytes(rng.choice(b"ACGTN") for _ in range(n))  # noqa: E731
    wrap = lambda s, w, eol: eol.join(s[i:i + w] for i in range(0, len(s), w))  # noqa: E731
    files = {}
    files["wrapped.fa"] = b"".join(b">chr%d some text\n" % i + wrap(seq(n), 60, b"\n") + b"\n" for i, n in enumerate([1000, 60, 61, 0, 5, 7000, 120]))
    files["crlf.fa"] = b"".join(b">r%d\r\n" % i + wrap(seq(n), 70, b"\r\n") + b"\r\n" for i, n in enumerate([300, 70, 1]))
    files["ragged.fa"] = b">a\nACGT\nAC\nACGTAC\n>b\nAAAA\nCCCC\nGG\n>c\n>d\nT\n"
    files["unwrapped.fa"] = b"".join(b">read%d\n" % i + seq(rng.randrange(1, 200)) + b"\n" for i in range(500))
    files["no_final_newline.fa"] = b">x\nACGT\nAC"
    edge = {
        "blank_inside.fa": b">a\nAC\n\nGT\n\n\n>b\n\nTT\n",
        "blank_between.fa": b">a\nACGT\n\n>b\nGG\n\n\n>c\nT\n",
        "gt_inside.fa": b">a>b desc>x\nAC>GT\nA>\n>c\nT>T\n",
        "header_last.fa": b">a\nACGT\n>last",
        "header_last_nl.fa": b">a\nACGT\n>last\n",
        "header_last_cr.fa": b">a\nACGT\n>last\r",
        "header_last_crlf.fa": b">a\nACGT\n>last\r\n",
        "cr_last.fa": b">a\r\nACGT\r\nAC\r",
        "empty_ids.fa": b">\nAC\n>\r\nGT\n>\n>\nT\n",
        "mixed_eol.fa": b">a x\r\nACGT\r\nAC\r\n>b\nGGTT\nGG\n>c\r\nT\nTT\r\nA\n",
        "only_header.fa": b">",
        "only_header_nl.fa": b">only\n",
        "empty.fa": b"",
    }
    files.update(edge)
    return files


def test_definition_equals_the_host_reader(tmp_path):
    from sassy_amd.fastx import read_fastx_batches
    for name, data in corpus().items():
        (tmp_path / name).write_bytes(data)
        want = fasta_ref.ids_and_sequences(data)
        for bb in (64, 1000, 1 << 20):
            got = []
            for rb in read_fastx_batches(str(tmp_path / name), bb):
                got += [(rb.id(i), rb.sequence(i)) for i in range(len(rb))]
            assert got == want, (name, bb, got[:3], want[:3])


def test_definition_on_a_case_written_out_by_hand():
    raw = b">r1 d\r\nAC\r\nG\rT\r\n\n>\n>r3\nA>C\n>r4"
    recs = fasta_ref.parse(raw)
    assert [(raw[r.id_start:r.id_start + r.id_len], r.seq, r.seq_start) for r in recs] == \
        [(b"r1 d", b"ACG\rT", 0), (b"", b"", 64), (b"r3", b"A>C", 64), (b"r4", b"", 128)]
    text = fasta_ref.layout(recs)
    assert len(text) == 128 + 64 and text[:5] == b"ACG\rT" and text[64:67] == b"A>C" and not any(text[5:64]) and not any(text[67:])
    assert fasta_ref.parse(b"") == [] and fasta_ref.layout([]) == bytes(64)


def test_symbols_are_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(sassy.lib(), name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
    assert "} sassy_hip_FastaRecord;" in hdr and sassy.fasta_record_dtype().itemsize == 32
    assert len(sassy.lib().sassy_hip_fasta_unwrap.argtypes) == 5
    for name in ("DeviceFasta", "DeviceText"):
        assert hasattr(sassy, name), name
    from sassy_amd import fastx
    assert hasattr(fastx, "read_fasta_device_batches")
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"fasta_unwrap.hip"' in build and '"fasta_step.h"' in build


def test_device_text_is_what_the_text_arguments_read(sassy):
    t = sassy.DeviceText(0x1000, 37)
    addr, n, keep, on_dev = sassy._ptr_len(t)
    assert (addr, n, on_dev) == (0x1000, 37, True) and keep is t and t.dtype.itemsize == 1 and t.is_cuda


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal with its code and a message that names the reason, in a child that sees no device: a call that got as far
    as the device would say 'no usable HIP device' instead.  Then valid arguments: that message, loudly, from the C call, from
    DeviceFasta and from the reader."""
    code = r'''
import ctypes as C, os, sys, tempfile, sassy_amd
from sassy_amd import fastx
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
def call(raw, n=None, flags=0, out=True, addr=None):
    res = C.c_void_p(7)
    n = len(raw) if n is None else n
    rc = L.sassy_hip_fasta_unwrap(addr if addr is not None else raw, n, flags, None, C.byref(res) if out else None)
    return rc, L.sassy_hip_last_error().decode(), res.value
def refused(want, word, *a, **kw):
    rc, msg, res = call(*a, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (rc, msg, want, word)
    if kw.get("out", True):
        assert res is None, res  # nothing comes back
ok = b">a\nACGT\n"
refused(EINVAL, "null argument", None, n=8)
refused(EINVAL, "null argument", ok, out=False)
refused(EINVAL, "first byte is not '>'", b"ACGT\n")
refused(EINVAL, "first byte is not '>'", b"\n>a\nAC\n")
for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.ALL_MINIMA, sassy_amd.TEXT_UNCHANGED, sassy_amd.LINE_SPANS, 1 << 20,
              sassy_amd.TEXT_ON_DEVICE | sassy_amd.TEXT_UNCHANGED):
    refused(EINVAL, "fasta_unwrap takes SASSY_HIP_TEXT_ON_DEVICE only", ok, flags=flags)
for addr in (0x7000001, 0x7000008, 0x700000f):
    refused(EINVAL, "16-byte aligned", None, n=8, flags=sassy_amd.TEXT_ON_DEVICE, addr=addr)
refused(EUNSUPPORTED, "too long for the tile index", ok, n=1 << 47)  # (refused on its length: byte 0 is all that is read)
refused(EUNSUPPORTED, "too long for the tile index", None, n=(1 << 47) - 65535, flags=sassy_amd.TEXT_ON_DEVICE, addr=0x7000000)
assert L.sassy_hip_fasta_n_records(None) == 0 and L.sassy_hip_fasta_records(None) is None
assert L.sassy_hip_fasta_text(None) is None and L.sassy_hip_fasta_text_bytes(None) == 0
L.sassy_hip_fasta_free(None)
# valid arguments get as far as the device, and fail loudly there
for raw, kw in ((ok, {}), (b"", {}), (b">", {}), (None, dict(n=0)), (None, dict(n=(1 << 47) - 65536, flags=sassy_amd.TEXT_ON_DEVICE, addr=0x7000000))):
    rc, msg, res = call(raw, **kw)
    assert rc == ENODEVICE and "no usable HIP device" in msg and res is None, (rc, msg, res)
try:
    sassy_amd.DeviceFasta(ok)
except sassy_amd.SassyHipError as e:
    assert "no usable HIP device" in str(e), e
else:
    raise SystemExit(3)
d = tempfile.mkdtemp()
fa, fq = os.path.join(d, "a.fa"), os.path.join(d, "a.fq")
open(fa, "wb").write(ok); open(fq, "wb").write(b"@r\nACGT\n+\nIIII\n")
try:
    list(fastx.read_fasta_device_batches(fa))
except sassy_amd.SassyHipError as e:
    assert "no usable HIP device" in str(e), e
else:
    raise SystemExit(4)
try:
    list(fastx.read_fasta_device_batches(fq))
except ValueError as e:
    assert "read_fastx_batches" in str(e), e
else:
    raise SystemExit(5)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_step_arithmetic_against_brute_force_under_sanitizers(tmp_path):
    """tests/c/fasta_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: lanes over {A, \\n, \\r, >} at every density, length and carry-in against the byte-by-byte
    definition, summaries over random cuts and bracketings of a 4 KiB buffer, and whole inputs through the passes."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fasta_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "fasta_step_driver.cc")])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
        assert int(fields["lanes"]) == 6600 and int(fields["combines"]) == 280 and int(fields["pipelines"]) == 115


def test_step_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "fasta_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "__builtin_amdgcn" not in src
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>"]
    unit = open(os.path.join(ROOT, "sassy_amd", "csrc", "fasta_unwrap.hip")).read()
    assert '#include "fasta_step.h"' in unit and "asm" not in re.sub(r"//.*", "", unit)


def test_cli_takes_device_unwrap_where_the_calls_take_device_texts(sassy, capsys, monkeypatch):
    from sassy_amd import cli
    seen = {}
    monkeypatch.setattr(cli, "run_amplicon", lambda args, *a: seen.setdefault("amplicon", args) and 0)
    monkeypatch.setattr(cli, "run_count", lambda args, *a: seen.setdefault("count", args) and 0)
    monkeypatch.setattr(cli, "load_primers", lambda path: [])
    monkeypatch.setattr(cli, "load_count_patterns", lambda path: [])
    cli.main(["amplicon", "p.tsv", "g.fa", "-k", "1", "--min-len", "10", "--max-len", "100", "--device-unwrap", "--seq"])
    assert seen["amplicon"].device_unwrap and seen["amplicon"].seq
    cli.main(["count", "p.txt", "g.fa", "-k", "1", "--per-record", "--device-unwrap"])
    assert seen["count"].device_unwrap and seen["count"].per_record
    seen.clear()
    cli.main(["amplicon", "p.tsv", "g.fa", "-k", "1", "--min-len", "10", "--max-len", "100"])
    cli.main(["count", "p.txt", "g.fa", "-k", "1"])
    assert not seen["amplicon"].device_unwrap and not seen["count"].device_unwrap
    with pytest.raises(SystemExit):
        cli.main(["count", "p.txt", "g.fa", "-k", "1", "--device-unwrap"])
    assert "--per-record" in capsys.readouterr().err
    for cmd in ("search", "filter", "demux"):
        with pytest.raises(SystemExit):
            cli.main([cmd, "-p", "ACGT", "-k", "1", "--device-unwrap", "g.fa"])
        assert "--device-unwrap" in capsys.readouterr().err
