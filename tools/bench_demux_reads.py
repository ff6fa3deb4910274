"""Demultiplexing (DeviceReads.demux) over seeded synthetic reads -- 150 bases with kept qualities, one of 96 barcodes of 8 bases
(pairwise distance >= 3) at the 5' end, 1 % substitutions, a tenth of the reads with a random head instead of a barcode, Dna,
k = 1, min_delta = 1 -- with the read batch resident on the device.  Run it in a fresh process.

    python tools/bench_demux_reads.py [--reads 100000 1000000] [--reps 9] [--out profiles/demux_reads_bench.json]
    python tools/bench_demux_reads.py --trace-run         # the demux calls alone, for rocprofv3 --kernel-trace --stats

Per size, behind a warm-up of every leg whose result is checked against tests/helpers/demux_reads_ref.py on a sample and against
the numpy of the host route on all reads, the legs in turn, --reps times (median, min, max and (max - min) / median each):
  demux         DeviceReads.demux: between two device events, and by the host's clock as well (to set beside the host route)
  select        DeviceReads.select of one sample out of the sorted batch, by the host's clock
  host_route    what a user did without the call, by the host's clock: the text and the quality buffer downloaded, the
                definition in numpy over all reads at once (costs, best, second, the stable argsort, the clip), the sorted
                reads as FASTQ bytes, DeviceReads of them with kept qualities.  (The FASTQ is built by one numpy gather, which
                is faster than DeviceReads.from_sequences over a list: the route is measured at its best.)
  write_bytes   counted, not measured: what reads_window_write_kernel must move.  The kernels' times come from the kernel trace
                of a separate run (--trace-run).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from tools.bench_merge_pairs import fastq_bytes, merged_fastq, wall  # noqa: E402
from tools.bench_read_overlaps import HBM_PEAK, READ_LEN, Events, summary  # noqa: E402

N_BARCODES, M = 96, 8


def barcodes_apart(seed: int, count: int = N_BARCODES, m: int = M, dist: int = 3):
    """`count` seeded barcodes of m bases, every two at Hamming distance >= dist (greedy)."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = np.zeros((0, m), dtype=np.uint8)
    while len(out) < count:
        c = letters[rng.integers(0, 4, m)]
        if not len(out) or ((out != c[None, :]).sum(axis=1) >= dist).all():
            out = np.vstack([out, c[None, :]])
    return out


def synthetic_reads(n: int, seed: int, bcs):
    """(reads, qualities, planted sample or -1): two (n, 150) uint8 arrays."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = letters[rng.integers(0, 4, (n, READ_LEN))]
    which = rng.integers(0, len(bcs), n)
    planted = rng.random(n) >= 0.1
    reads[planted, :M] = bcs[which[planted]]
    subs = rng.random((n, READ_LEN)) < 0.01
    reads = np.where(subs, letters[rng.integers(0, 4, (n, READ_LEN))], reads).astype(np.uint8)
    quals = rng.integers(33, 75, (n, READ_LEN), dtype=np.uint8)
    return np.ascontiguousarray(reads), np.ascontiguousarray(quals), np.where(planted, which, -1)


def numpy_demux(reads, bcs, k: int, min_delta: int):
    """The definition over an (n, 150) array, the window at the 5' end: (labels, order, bounds, cost, second)."""
    n, B = len(reads), len(bcs)
    costs = np.zeros((n, B), dtype=np.uint8)
    win = reads[:, :M]
    for j in range(B):
        costs[:, j] = (win != bcs[j][None, :]).sum(axis=1)
    best = costs.argmin(axis=1)
    rows = np.arange(n)
    cost = costs[rows, best].astype(np.int64)
    costs[rows, best] = M + 1
    second = costs.min(axis=1).astype(np.int64) if B > 1 else np.full(n, M + 1, dtype=np.int64)
    assigned = (cost <= k) & (second - cost >= min_delta)
    labels = np.where(assigned, best, B)
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(B + 2), side="left")
    return labels, order, bounds, cost, second


def run_size(sassy_amd, n, a, trace_only=False):
    import demux_reads_ref as dref
    bcs = barcodes_apart(a.seed)
    barcodes = [b.tobytes() for b in bcs]
    reads, quals, planted = synthetic_reads(n, a.seed + 1, bcs)
    s = sassy_amd.Searcher("dna", rc=False)
    h = sassy_amd.DeviceReads(fastq_bytes(reads, quals), keep_quality=True)
    call = dict(k=a.k, min_delta=a.min_delta)

    def host_route():
        t = np.frombuffer(h.download_text(), dtype=np.uint8)[:n * 192].reshape(n, 192)[:, :READ_LEN]  # (150 bases: a slot of 192 bytes)
        q = np.frombuffer(h.download_quality_text(), dtype=np.uint8)[:n * 192].reshape(n, 192)[:, :READ_LEN]
        labels, order, bounds, _, _ = numpy_demux(t, bcs, a.k, a.min_delta)
        clip = labels[order] < len(bcs)
        ts, qs = t[order], q[order]
        ts[clip, :READ_LEN - M], qs[clip, :READ_LEN - M] = ts[clip, M:], qs[clip, M:]
        lens = np.where(clip, READ_LEN - M, READ_LEN)
        return sassy_amd.DeviceReads(merged_fastq(ts, qs, lens), keep_quality=True), (order, bounds)

    # warm-up of every leg, and the checks
    d = h.demux(s, barcodes, with_records=True, **call)
    sample = np.random.default_rng(1).choice(n, 300, replace=False).tolist()
    want = dref.expected_demux("dna", [(reads[i].tobytes(), quals[i].tobytes()) for i in sample], barcodes, **call)
    for f in ("sample", "best", "cost", "second", "n_best"):
        assert np.array_equal(d.records[f][sample], want[0][f]), "the call's records and the definition disagree: " + f
    if trace_only:  # (the kernels of the demux alone)
        d.free()
        for _ in range(a.reps):
            h.demux(s, barcodes, **call).free()
        h.free()
        return None
    routed, (order, bounds) = host_route()
    assert np.array_equal(order.astype(np.uint64), d.order) and np.array_equal(bounds.astype(np.uint64), d.bounds), "the host route sorts otherwise"
    assert routed.download_text() == d.reads.download_text() and routed.download_quality_text() == d.reads.download_quality_text(), "the host route clips otherwise"
    routed.free()
    layout, kept_bases = int(d.reads.text_bytes), int(d.reads.seq_lens.sum())
    counts = d.counts
    big = int(np.argmax(counts[:-1]))
    one = d.sample(big)
    sample_records, sample_layout = len(one), int(one.text_bytes)
    one.free()
    rec = d.records
    events = Events()
    t = {k: [] for k in ("demux_events", "demux_wall", "select_wall", "host_route")}
    for _ in range(a.reps):
        d.free()
        events.start()
        d, ms = wall(lambda: h.demux(s, barcodes, **call))
        t["demux_events"].append(events.stop_ms())
        t["demux_wall"].append(ms)
        one, ms = wall(lambda: d.sample(big))
        t["select_wall"].append(ms)
        one.free()
        (routed, _), ms = wall(host_route)
        t["host_route"].append(ms)
        routed.free()
    d.free()
    h.free()
    blocks = (layout - 64) // 64
    # what the write kernel reads of text and quality, what it writes of both and of the block table, and per record its source,
    # its begin and its two table entries
    write_bytes = 2 * kept_bases + 2 * layout + 4 * blocks + (8 + 8 + 16 + 8) * n
    b, c = statistics.median(t["demux_wall"]), statistics.median(t["host_route"])
    beyond = max(t["demux_wall"]) < min(t["host_route"]) or min(t["demux_wall"]) > max(t["host_route"])
    return {
        "input": {"reads": n, "read_len": READ_LEN, "barcodes": N_BARCODES, "barcode_len": M, "min_pairwise_distance": 3, "substitutions": 0.01,
                  "random_heads": 0.1, "end": "5'", "at": 0, **call, "seed": a.seed},
        "result": {"assigned": int((rec["sample"] >= 0).sum()), "assigned_to_the_planted": int(((rec["sample"] == planted) & (planted >= 0)).sum()),
                   "cost_1": int(((rec["sample"] >= 0) & (rec["cost"] == 1)).sum()), "unassigned": int(counts[-1]), "layout_bytes": layout,
                   "kept_bases": kept_bases, "largest_sample": {"index": big, "records": sample_records, "layout_bytes": sample_layout}},
        "ms": {k: summary(v) for k, v in t.items()},
        "host_route_over_demux": round(c / b, 2), "ranges_apart": bool(beyond),
        "write_bytes": write_bytes, "write_ms_at_peak": round(write_bytes / HBM_PEAK * 1e3, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("-k", type=int, default=1)
    ap.add_argument("--min-delta", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--trace-run", action="store_true", help="warm-up and --reps demux calls per size, nothing written: the run a kernel trace wraps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demux_reads_bench.json"))
    a = ap.parse_args()
    import sassy_amd
    if sassy_amd.device_count() == 0:
        raise SystemExit("no HIP device visible: nothing is measured without one")
    if a.trace_run:
        for n in a.reads:
            run_size(sassy_amd, n, a, trace_only=True)
        return 0
    out = {"reps": a.reps, "version": sassy_amd.lib().sassy_hip_version().decode(), "sizes": [run_size(sassy_amd, n, a) for n in a.reads]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
