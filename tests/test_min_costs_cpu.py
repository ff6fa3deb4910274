"""CPU-only: the best-cost search's surface (sassy_hip_min_costs / sassy_hip_best_pattern, Searcher.min_costs /
.best_pattern, `python -m sassy_amd filter`) -- what needs no device: the symbols, the argument errors that come before
any device work, the loud failure without a device, the CLI's record writer and -v logic against a stubbed cost array,
FASTQ quality lines through the batch reader."""
import ctypes as C
import gzip
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sassy_hip_min_costs", "sassy_hip_best_pattern")


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
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(sassy.lib(), name), name
        assert name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", rust), name
    assert re.search(r"#define\s+SASSY_HIP_NO_MATCH\s+255u", hdr) and sassy.NO_MATCH == 255
    names = [r[0] for r in sassy.option_table()]
    assert "min_cost_device" in names


def test_argument_errors_come_before_any_device_work(sassy):
    """k = 255, a foreign flag and a null output are SASSY_HIP_EINVAL whether or not the box has a device (the child sees
    none: a call that got as far as the device would say 'no usable HIP device' instead)."""
    code = (
        "import ctypes as C, sassy_amd\n"
        "L = sassy_amd.lib()\n"
        "s = sassy_amd.Searcher('iupac', rc=True)\n"
        "pats, texts = [b'ACGTACGTAC', b'TTGACCATGA'], [b'ACGTACGTACGT', b'GGGG', b'']\n"
        "pp = (C.c_char_p * 2)(*pats); pl = (C.c_size_t * 2)(10, 10)\n"
        "tp = (C.c_char_p * 3)(*texts); tp = C.cast(tp, C.POINTER(C.c_void_p)); tl = (C.c_size_t * 3)(12, 4, 0)\n"
        "cost = (C.c_uint8 * 6)(); pat = (C.c_uint32 * 3)(); strand = (C.c_uint8 * 6)()\n"
        "def err():\n"
        "    return L.sassy_hip_last_error().decode()\n"
        "for k, flags, out in ((255, 0, cost), (1, sassy_amd.ALL_MINIMA, cost), (1, sassy_amd.WITHOUT_TRACE, cost), (1, 8, cost), (1, 0, None)):\n"
        "    assert L.sassy_hip_min_costs(s._h, pp, pl, 2, tp, tl, 3, k, flags, out, strand) == -1, (k, flags, err())\n"
        "    assert 'no usable HIP device' not in err(), err()\n"
        "    assert L.sassy_hip_best_pattern(s._h, pp, pl, 2, tp, tl, 3, k, flags, out, pat, strand) == -1, (k, flags, err())\n"
        "assert L.sassy_hip_min_costs(None, pp, pl, 2, tp, tl, 3, 1, 0, cost, strand) == -1\n"
        "assert L.sassy_hip_best_pattern(s._h, None, pl, 2, tp, tl, 3, 1, 0, cost, pat, strand) == -1\n"
        # valid arguments: only now the device is asked for
        "assert L.sassy_hip_min_costs(s._h, pp, pl, 2, tp, tl, 3, 1, 0, cost, None) == -2 and 'no usable HIP device' in err(), err()\n"
        "assert L.sassy_hip_best_pattern(s._h, pp, pl, 2, tp, tl, 3, 1, 0, cost, None, None) == -2 and 'no usable HIP device' in err(), err()\n"
        "try:\n    s.min_costs(pats, texts, 300)\nexcept sassy_amd.SassyHipError as e:\n    assert 'k must be <= 254' in str(e), e\nelse:\n    raise SystemExit(3)\n"
        "print('ok')\n"
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_no_device_fails_loudly(sassy):
    """No fall-back of any kind: without a device both calls raise, with both settings of min_cost_device, for a list and
    for a TextBatch (child process that sees no HIP device, as tests/test_cabi_symbols.py does it)."""
    code = (
        "import re, sassy_amd\n"
        "assert sassy_amd.device_count() == 0\n"
        "pats, texts = [b'ACGTACGTAC'] * 4, [b'ACGTACGTACGT', b'GGGG']\n"
        "for dev in (1, 0):\n"
        "    for alphabet, rc in (('dna', False), ('iupac', True), ('ascii', False)):\n"
        "        s = sassy_amd.Searcher(alphabet, rc=rc)\n"
        "        s.set_option('min_cost_device', dev)\n"
        "        for f in (s.min_costs, s.best_pattern):\n"
        "            for tx in (texts, sassy_amd.TextBatch.from_list(texts)):\n"
        "                try:\n"
        "                    f(pats, tx, 1)\n"
        "                except sassy_amd.SassyHipError as e:\n"
        "                    assert re.search('no usable HIP device', str(e)), e\n"
        "                else:\n"
        "                    raise AssertionError('no SassyHipError')\n"
        "print('ok')\n"
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


FASTQ = b"@r1 first\nACGTN\n+\nIIII#\n@r2\nGG\n+\n@I\n@r3 x y\nTTTTTTTT\n+r3\n!!!!!!!!\n"
FASTA_WRAPPED = b">chr1 desc\nACGT\nACGT\nAC\n>chr2\nTTTT\n>empty\n>chr4\nGGGGCCCC\nAA\n"


def _records(path, batch_bytes):
    from sassy_amd.fastx import read_fastx_batches
    out = []
    for rb in read_fastx_batches(path, batch_bytes):
        out += [(rb.id(i), rb.sequence(i), rb.quality(i), rb.is_fastq) for i in range(len(rb))]
    return out


def test_fastq_qualities_round_trip_through_the_batch_reader(sassy, tmp_path):
    """The quality line is an offset / length pair into the file's bytes: plain, gzip, CRLF, no final newline, batches
    smaller than a record; FASTA records have none."""
    want = [("r1 first", b"ACGTN", b"IIII#", True), ("r2", b"GG", b"@I", True), ("r3 x y", b"TTTTTTTT", b"!!!!!!!!", True)]
    files = {"plain.fq": FASTQ, "crlf.fq": FASTQ.replace(b"\n", b"\r\n"), "no_final_newline.fq": FASTQ[:-1]}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    with gzip.open(tmp_path / "reads.fq.gz", "wb") as fh:
        fh.write(FASTQ)
    for name in list(files) + ["reads.fq.gz"]:
        for bb in (8, 40, 1 << 20):
            assert _records(str(tmp_path / name), bb) == want, (name, bb)
    (tmp_path / "a.fa").write_bytes(FASTA_WRAPPED)
    got = _records(str(tmp_path / "a.fa"), 1 << 20)
    assert got == [("chr1 desc", b"ACGTACGTAC", None, False), ("chr2", b"TTTT", None, False), ("empty", b"", None, False),
                   ("chr4", b"GGGGCCCCAA", None, False)]


def test_filter_record_writer_and_invert_against_a_stubbed_cost_array(sassy, tmp_path, capsysbinary):
    """`filter` with a searcher whose best_pattern is a stub: the records whose cost is a match, in input order, in the
    reference's record shape (FASTQ: @id / sequence / + / quality; FASTA: >id / sequence on one line); -v: the others;
    the two outputs partition the input."""
    from sassy_amd import cli
    (tmp_path / "r.fq").write_bytes(FASTQ.replace(b"+r3\n", b"+\n"))
    (tmp_path / "w.fa").write_bytes(FASTA_WRAPPED)
    seen = []

    class Stub:
        def __init__(self, *a, **kw):
            seen.append((a, kw))

        def with_max_n_frac(self, f):
            seen.append(("max_n_frac", f))
            return self

        def best_pattern(self, pats, texts, k):
            n = len(texts)
            cost = np.full(n, sassy.NO_MATCH, dtype=np.uint8)
            cost[0::2] = np.arange(len(cost[0::2]))  # records 0, 2, ... match (cost 0 is a match too)
            return cost, np.zeros(n, np.uint32), np.zeros(n, np.uint8)

    real = cli.Searcher
    cli.Searcher = Stub
    try:
        def run(*argv):
            assert cli.main(list(argv)) == 0
            return capsysbinary.readouterr().out
        fq, fa = str(tmp_path / "r.fq"), str(tmp_path / "w.fa")
        assert run("filter", "-p", "ACGT", "-k", "1", fq) == b"@r1 first\nACGTN\n+\nIIII#\n@r3 x y\nTTTTTTTT\n+\n!!!!!!!!\n"
        assert run("filter", "-p", "ACGT", "-k", "1", "-v", fq) == b"@r2\nGG\n+\n@I\n"
        assert run("filter", "-p", "ACGT", "-k", "1", fa) == b">chr1 desc\nACGTACGTAC\n>empty\n\n"
        assert run("filter", "-p", "ACGT", "-k", "1", "--invert", fa) == b">chr2\nTTTT\n>chr4\nGGGGCCCCAA\n"
        # several files, in argument order; the searcher settings are `search`'s
        seen.clear()
        assert run("filter", "-p", "ACGT", "-k", "0", "-a", "dna", "--no-rc", "--max-n-frac", "0.5", fa, fq).startswith(b">chr1 desc\n")
        assert seen == [(("dna",), {"rc": False, "alpha": None}), ("max_n_frac", 0.5)]
    finally:
        cli.Searcher = real
    assert list(cli.kept_records(np.array([0, 255, 3, 255], np.uint8), False)) == [0, 2]
    assert list(cli.kept_records(np.array([0, 255, 3, 255], np.uint8), True)) == [1, 3]
    out = io.BytesIO()
    from sassy_amd.fastx import read_fastx_batches
    for rb in read_fastx_batches(str(tmp_path / "r.fq"), 1 << 20):
        cli.write_records(out, rb, range(len(rb)))
    assert out.getvalue() == FASTQ.replace(b"+r3\n", b"+\n")
