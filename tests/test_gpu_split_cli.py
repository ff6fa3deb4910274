"""`python -m sassy_amd split` on a small FASTQ pair: the files it writes are what the definition
(tests/helpers/demux_reads_ref.py) and the four-line format of `reads_to_fastq` give -- one file per barcode and `unassigned`,
the mates whole in the same order under `_2`, the records as TSV."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import demux_reads_ref as dref  # noqa: E402

pytestmark = pytest.mark.gpu

BARCODES = [b"ACGTACGT", b"ACGTACAA", b"TTGGCCAA", b"GGATTCCA"]
NAMES = ["alpha", "beta", "gamma", "delta"]


def fastq(ids, reads):
    return b"".join(b"@" + i.encode() + b"\n" + s + b"\n+\n" + q + b"\n" for i, (s, q) in zip(ids, reads) if s)


@pytest.mark.parametrize("extra,kw", [([], {}), (["--at", "2", "--end3", "--keep-barcode", "--min-delta", "0"], dict(at=2, end3=True, clip=False, min_delta=0))])
def test_split_writes_what_the_definition_gives(tmp_path, extra, kw):
    rng = np.random.default_rng(17)
    reads = dref.mixed_batch(200, 13, BARCODES, at=kw.get("at", 0), end3=kw.get("end3", False))
    reads = [(s, q) if s else (b"A", b"I") for s, q in reads]   # (four-line FASTQ with an empty sequence line is still a record; keep it simple)
    mates = [(bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).astype(np.uint8)), b"F" * n) for n in rng.integers(1, 90, len(reads)).tolist()]
    ids = [f"read{i} lane=1" for i in range(len(reads))]
    ids2 = [f"read{i} lane=2" for i in range(len(reads))]
    (tmp_path / "r1.fq").write_bytes(fastq(ids, reads))
    (tmp_path / "r2.fq").write_bytes(fastq(ids2, mates))
    (tmp_path / "bc.fa").write_bytes(b"".join(b">" + n.encode() + b" sample\n" + b + b"\n" for n, b in zip(NAMES, BARCODES)))
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "sassy_amd", "split", str(tmp_path / "r1.fq"), "-f", str(tmp_path / "bc.fa"), "-k", "1", "-o", str(out),
                        "--mate", str(tmp_path / "r2.fq"), "--tsv"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    records, order, bounds, seqs, quals = dref.expected_demux("dna", reads, BARCODES, k=1, **dict(dict(min_delta=1), **kw))
    order = order.astype(np.int64).tolist()
    names = NAMES + ["unassigned"]
    assert sorted(os.listdir(out)) == sorted([n + ".fq" for n in names] + [n + "_2.fq" for n in names] + ["assignments.tsv"])
    written = 0
    for s, name in enumerate(names):
        a, b = int(bounds[s]), int(bounds[s + 1])
        want1 = fastq([ids[r] for r in order[a:b]], list(zip(seqs[a:b], quals[a:b])))
        want2 = fastq([ids2[r] for r in order[a:b]], [mates[r] for r in order[a:b]])
        assert (out / (name + ".fq")).read_bytes() == want1, name
        assert (out / (name + "_2.fq")).read_bytes() == want2, name
        written += b - a
    assert written == len(reads) and all(int(bounds[s + 1]) - int(bounds[s]) >= 10 for s in range(5))
    rows = (out / "assignments.tsv").read_text().splitlines()
    assert rows[0] == "id\tsample\tbest\tcost\tsecond\tn_best" and len(rows) == 1 + len(reads)
    for i, (row, r) in enumerate(zip(rows[1:], records)):
        sample = names[int(r["sample"])] if r["sample"] >= 0 else "unassigned"
        best = int(r["best"]) if r["n_best"] else -1
        assert row == f"{ids[i]}\t{sample}\t{best}\t{int(r['cost'])}\t{int(r['second'])}\t{int(r['n_best'])}", (i, row)
