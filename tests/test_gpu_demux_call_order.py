"""Call order: a demux between two calls of other families on ONE searcher changes neither's result, and the demux's own result
does not depend on what ran in front of it.  The demux keeps its barcode table, its records and the sort's scratch in buffers of
the searcher and runs the Dna look, the sort and the layout scan on the searcher's stream, which the other families use as
well."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import demux_reads_ref as dref  # noqa: E402
import read_overlaps_ref as oref  # noqa: E402

pytestmark = pytest.mark.gpu

AD = b"AGATCGGAAGAGCACACGTC"
BARCODES = [b"ACGTACGT", b"ACGTACAA", b"TTGGCCAA", b"GGATTCCA"]


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


def test_a_demux_between_calls_of_other_families(sassy):
    rng = np.random.default_rng(6)
    reads = [(s, q) for s, q in dref.mixed_batch(120, 9, BARCODES) if len(s) >= 40][:50]
    assert len(reads) == 50
    seqs = [s for s, _ in reads]
    mates = [oref.revcomp("dna", s[-30:]) for s in seqs]
    pats = [seqs[0][3:15], seqs[7][10:22], b"ACGTACGTACGT"]
    text = b"".join(seqs)
    key = lambda m: (m.pattern_idx, getattr(m, "text_idx", 0), m.text_start, m.text_end, m.cost, m.strand, m.cigar)  # noqa: E731
    batch = dref.mixed_batch(300, 10, BARCODES)
    want = dref.expected_demux("dna", batch, BARCODES, k=1, min_delta=1)

    def demux(s):
        d = sassy.demux_reads(s, batch, BARCODES, k=1, min_delta=1, with_records=True)
        out = (d.records.tobytes(), d.order.tobytes(), d.bounds.tobytes(), d.reads.download_text(), d.reads.download_quality_text(),
               d.reads.download_rem().tobytes())
        d.free()
        return out

    def trim(s):
        trimmed, records = s.trim_reads(reads, [AD], 4, 2, 100, 15, 20, with_records=True)
        out = (records.tobytes(), trimmed.download_text(), trimmed.download_quality_text())
        trimmed.free()
        return out

    families = {
        "search": lambda s: [key(m) for m in s.search(pats[0], text, 1)],
        "search_many": lambda s: [key(m) for m in s.search_many(pats, seqs, 2)],
        "hamming_best_pattern": lambda s: [a.tolist() for a in s.hamming_best_pattern(pats, seqs, 2)],
        "read_overlaps": lambda s: s.read_overlaps(seqs, mates, 10, 2, 100).tobytes(),
        "merge_pairs": lambda s: (lambda m: (m.download_text(), m.free())[0])(s.merge_pairs(reads, [(m, b"I" * len(m)) for m in mates], 10, 2, 100)),
        "trim_reads": trim,
    }
    fresh = {name: fn(sassy.Searcher("dna", rc=False)) for name, fn in families.items()}
    alone = demux(sassy.Searcher("dna", rc=False))
    assert alone[0] == want[0].tobytes() and alone[1] == want[1].tobytes() and alone[2] == want[2].tobytes()
    assert all(v >= 30 for v in dref.groups(want[0], 1).values())
    assert len(fresh["search_many"]) > 2 and len(fresh["search"]) > 0
    names = list(families)
    for i, before in enumerate(names):
        after = names[(i + 1) % len(names)]
        s = sassy.Searcher("dna", rc=False)
        assert families[before](s) == fresh[before], before
        assert demux(s) == alone, ("the demux behind", before)
        assert families[after](s) == fresh[after], (after, "behind a demux")
        assert families[before](s) == fresh[before], (before, "again")
        assert demux(s) == alone, ("the demux again, behind", before)
