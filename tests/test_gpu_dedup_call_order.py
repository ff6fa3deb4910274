"""Call order: a dedup between two calls of other families on ONE searcher changes neither's result, and the dedup's own result
does not depend on what ran in front of it.  The dedup writes the pair family's plane buffers (d_pairs_a, d_pairs_t) from a
kernel, runs the grouping's device part in the grouping's own buffers (d_umi_reads, d_umi_distinct) and the Dna look, the scans
and the layout scan on the searcher's stream: `Searcher.umi_groups`, `hamming_pairs` and `hamming_clusters` use the same
buffers, the other families the same stream."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, ROOT)

import dedup_reads_ref as ddref  # noqa: E402
import demux_reads_ref as dref  # noqa: E402
import read_overlaps_ref as oref  # noqa: E402
import umi_groups_ref as uref  # noqa: E402

pytestmark = pytest.mark.gpu

AD = b"AGATCGGAAGAGCACACGTC"
BARCODES = [b"ACGTACGT", b"ACGTACAA", b"TTGGCCAA", b"GGATTCCA"]


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


@pytest.mark.parametrize("rc", [False, True])
def test_a_dedup_between_calls_of_other_families(sassy, rc):
    reads = [(s, q) for s, q in dref.mixed_batch(120, 9, BARCODES) if len(s) >= 40][:50]
    assert len(reads) == 50
    seqs = [s for s, _ in reads]
    mates = [oref.revcomp("dna", s[-30:]) for s in seqs]
    pats = [seqs[0][3:15], seqs[7][10:22], b"ACGTACGTACGT"]
    text = b"".join(seqs)
    key = lambda m: (m.pattern_idx, getattr(m, "text_idx", 0), m.text_start, m.text_end, m.cost, m.strand, m.cigar)  # noqa: E731
    batch = ddref.seeded_batch(600, 21, rc_mix=rc, n_umis=30)
    want = ddref.expected_dedup("dna", batch, 12, rc=rc)
    # another list for the host grouping than the dedup's own windows, of another length and count: what it leaves in the shared
    # buffers is not what the dedup needs
    umis = [s[:9] for s, _ in ddref.seeded_batch(400, 22, m=9, n_umis=25) if len(s) >= 9]
    want_umis = uref.expected_umi_groups("dna", umis, 1, "directional", rc=rc)

    def dedup(s):
        d = sassy.dedup_reads(s, batch, 12, with_columns=True)
        out = (d.label.tobytes(), d.size.tobytes(), d.rep.tobytes(), d.count.tobytes(), d.kept.tobytes(), d.n_unique, d.n_groups, d.reads.download_text(),
               d.reads.download_quality_text(), d.reads.download_rem().tobytes())
        d.free()
        return out

    def groups_reads(s):
        b = sassy.DeviceReads.from_sequences([x[0] for x in batch])
        try:
            g = b.umi_groups(s, 12, method="cluster", end3=False)
            return tuple(a.tobytes() for a in g[:4]) + g[4:]
        finally:
            b.free()

    def trim(s):
        trimmed, records = s.trim_reads(reads, [AD], 4, 2, 100, 15, 20, with_records=True)
        out = (records.tobytes(), trimmed.download_text(), trimmed.download_quality_text())
        trimmed.free()
        return out

    def demux(s):
        d = sassy.demux_reads(s, reads, BARCODES, k=1, min_delta=1, with_records=True)
        out = (d.records.tobytes(), d.order.tobytes(), d.bounds.tobytes(), d.reads.download_text())
        d.free()
        return out

    families = {
        "umi_groups": lambda s: tuple(a.tobytes() for a in s.umi_groups(umis, 1, "directional")),
        "umi_groups_cluster": lambda s: tuple(a.tobytes() for a in s.umi_groups(umis, 2, "cluster")),
        "hamming_pairs": lambda s: s.hamming_pairs(umis[:150], None, 1).tobytes(),
        "hamming_clusters": lambda s: tuple(a.tobytes() for a in s.hamming_clusters(umis, 1)),
        "umi_groups_reads": groups_reads,
        "search": lambda s: [key(m) for m in s.search(pats[0], text, 1)],
        "search_many": lambda s: [key(m) for m in s.search_many(pats, seqs, 2)],
        "hamming_best_pattern": lambda s: [a.tolist() for a in s.hamming_best_pattern(pats, seqs, 2)],
        "read_overlaps": lambda s: s.read_overlaps(seqs, mates, 10, 2, 100).tobytes(),
        "merge_pairs": lambda s: (lambda m: (m.download_text(), m.free())[0])(s.merge_pairs(reads, [(m, b"I" * len(m)) for m in mates], 10, 2, 100)),
        "trim_reads": trim,
        "demux_reads": demux,
    }
    fresh = {name: fn(sassy.Searcher("dna", rc=rc)) for name, fn in families.items()}
    alone = dedup(sassy.Searcher("dna", rc=rc))
    assert alone[:5] == tuple(a.tobytes() for a in want[:4]) + (want[6].tobytes(),) and alone[5:7] == want[4:6]
    assert fresh["umi_groups"] == tuple(a.tobytes() for a in want_umis)
    described = ddref.describe("dna", batch, 12, rc=rc)
    assert described["mixed_groups"] > 10 and described["no_window"] > 30 and described["score_ties"] > 0, described
    assert len(fresh["search_many"]) > 2 and len(fresh["search"]) > 0 and len(fresh["hamming_pairs"]) > 0
    names = list(families)
    for i, before in enumerate(names):
        after = names[(i + 1) % len(names)]
        s = sassy.Searcher("dna", rc=rc)
        assert families[before](s) == fresh[before], before
        assert dedup(s) == alone, ("the dedup behind", before)
        assert families[after](s) == fresh[after], (after, "behind a dedup")
        assert families[before](s) == fresh[before], (before, "again")
        assert dedup(s) == alone, ("the dedup again, behind", before)
