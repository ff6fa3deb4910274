"""Paired-end merge (Searcher.merge_pairs) over the seeded synthetic pairs of tools/bench_read_overlaps.py -- 150-base reads cut
from fragments of 50 .. 400 bases, 1 % substitutions, Dna, min_overlap 10, max_permille 200, k open -- with qualities drawn
from 33 .. 74 and both read batches resident on the device.  Run it in a fresh process.

    python tools/bench_merge_pairs.py [--pairs 100000 1000000] [--reps 9] [--out profiles/merge_pairs_bench.json]
    python tools/bench_merge_pairs.py --trace-run          # the merge calls alone, for rocprofv3 --kernel-trace --stats

Per size, behind a warm-up of every leg whose merged reads are checked on a sample against tests/helpers/merge_pairs_ref.py,
the legs in turn, --reps times (median, min, max and (max - min) / median each):
  overlaps     (a) Searcher.read_overlaps alone, the records on the host: the floor, and all the parent commit can do on the device
  merge        (b) Searcher.merge_pairs: between two device events, and by the host's clock as well (to set beside (c))
  host_route   (c) what a user did without the call, by the host's clock: read_overlaps, both sequence buffers downloaded, a
               numpy merge over all pairs at once (the qualities are the host's own copy), the merged reads as FASTQ bytes,
               DeviceReads of them with kept qualities
  scan_merged  (d) hamming_best_pattern (16 patterns of 12 bases, k = 1) on the merged handle, and the same call on the host
               list of the merged reads, by the host's clock
  write_bytes  counted, not measured: what merge_write_kernel must move -- per merged pair both reads and both qualities once,
               the merged text and quality layouts written once, 4 bytes of rem per block, 16 bytes of record, 48 bytes of
               tables per pair.  Its kernel time comes from the kernel trace of a separate run (--trace-run).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from tools.bench_read_overlaps import COMP, HBM_PEAK, READ_LEN, Events, summary, synthetic_pairs  # noqa: E402


def fastq_bytes(reads: np.ndarray, quals: np.ndarray) -> np.ndarray:
    """four-line FASTQ of two (n, L) arrays: '@', the bases, '+', the qualities"""
    n, L = reads.shape
    grid = np.empty((n, 2 * L + 6), dtype=np.uint8)
    grid[:, :2] = np.frombuffer(b"@\n", dtype=np.uint8)
    grid[:, 2:2 + L] = reads
    grid[:, 2 + L:5 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    grid[:, 5 + L:5 + 2 * L] = quals
    grid[:, 5 + 2 * L] = 10
    return grid.reshape(-1)


def numpy_merge(r1, q1, r2, q2, rec, chunk=1 << 16):
    """The definition over (n, 150) arrays, 65 536 pairs at a time with 16-bit indices: (text, quality, lengths), the first two
    (n, 300) with the columns behind a pair's length unset."""
    n, L = r1.shape
    off = rec["offset"].astype(np.int64)
    lens = np.where(rec["n_accepted"] == 0, 0, np.where(off >= 0, np.maximum(L, off + L), rec["overlap"])).astype(np.int64)
    text, qual = np.empty((n, 2 * L), dtype=np.uint8), np.empty((n, 2 * L), dtype=np.uint8)
    p = np.arange(2 * L, dtype=np.int16)[None, :]
    in_a, ia = p < L, np.minimum(p, L - 1)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        j = p - off[lo:hi, None].astype(np.int16)
        in_b = (j >= 0) & (j < L)
        rows = np.arange(hi - lo)[:, None]
        ib = (L - 1) - np.clip(j, 0, L - 1)  # b[j] is the complement of R2's byte L - 1 - j
        ca, xa = r1[lo:hi][rows, ia], q1[lo:hi][rows, ia].astype(np.int16)
        cb, xb = COMP[r2[lo:hi][rows, ib]], q2[lo:hi][rows, ib].astype(np.int16)
        both, a_wins = in_a & in_b, xa >= xb
        text[lo:hi] = np.where(both, np.where(a_wins, ca, cb), np.where(in_a, ca, cb))
        q_both = np.where(ca == cb, np.maximum(xa, xb), np.minimum(126, 33 + np.maximum(2, np.abs(xa - xb))))
        qual[lo:hi] = np.where(both, q_both, np.where(in_a, xa, xb))
    return text, qual, lens


def merged_fastq(text, qual, lens) -> bytes:
    """FASTQ of numpy_merge's result, a record per pair (an unmerged pair: an empty read)."""
    n, W = text.shape
    grid = np.empty((n, 2 * W + 6), dtype=np.uint8)
    keep = np.zeros((n, 2 * W + 6), dtype=bool)
    live = np.arange(W)[None, :] < lens[:, None]
    grid[:, :2] = np.frombuffer(b"@\n", dtype=np.uint8)
    grid[:, 2:2 + W] = text
    grid[:, 2 + W:5 + W] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    grid[:, 5 + W:5 + 2 * W] = qual
    grid[:, 5 + 2 * W] = 10
    keep[:, :2] = keep[:, 2 + W:5 + W] = True
    keep[:, 5 + 2 * W] = True
    keep[:, 2:2 + W] = keep[:, 5 + W:5 + 2 * W] = live
    return grid[keep].tobytes()


def wall(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def run_size(sassy_amd, n, a, trace_only=False):
    import merge_pairs_ref as mref
    r1, r2, _ = synthetic_pairs(n, a.seed)
    rng = np.random.default_rng(a.seed + 1)
    q1, q2 = rng.integers(33, 75, r1.shape, dtype=np.uint8), rng.integers(33, 75, r2.shape, dtype=np.uint8)
    s = sassy_amd.Searcher("dna", rc=False)
    scan = sassy_amd.Searcher("dna", rc=True)
    h1 = sassy_amd.DeviceReads(fastq_bytes(r1, q1), keep_quality=True)
    h2 = sassy_amd.DeviceReads(fastq_bytes(r2, q2), keep_quality=True)
    args = (a.min_overlap, 512, a.max_permille)
    pats = [bytes(np.random.default_rng(7 + i).choice(np.frombuffer(b"ACGT", dtype=np.uint8), 12).astype(np.uint8)) for i in range(16)]

    def host_route():
        rec = s.read_overlaps(h1, h2, *args)
        t1 = np.frombuffer(h1.download_text(), dtype=np.uint8)
        t2 = np.frombuffer(h2.download_text(), dtype=np.uint8)
        # (every read is 150 bases: its slot is 192 bytes of the layout)
        a1, a2 = t1[:n * 192].reshape(n, 192)[:, :READ_LEN], t2[:n * 192].reshape(n, 192)[:, :READ_LEN]
        text, qual, lens = numpy_merge(a1, q1, a2, q2, rec)
        return sassy_amd.DeviceReads(merged_fastq(text, qual, lens), keep_quality=True), (text, qual, lens)

    # warm-up of every leg, and the check on a sample
    merged, rec = s.merge_pairs(h1, h2, *args, with_overlaps=True)
    sample = np.random.default_rng(1).choice(n, 300, replace=False).tolist()
    want = mref.expected_merge("dna", [(r1[i].tobytes(), q1[i].tobytes()) for i in sample], [(r2[i].tobytes(), q2[i].tobytes()) for i in sample], *args)
    assert np.array_equal(rec[sample], want[0]), "the call's records and the definition disagree"
    assert [merged.download(i) for i in sample] == want[1] and [merged.quality(i) for i in sample] == want[2], "the merge and the definition disagree"
    if trace_only:  # (the kernels of the merge alone)
        merged.free()
        for _ in range(a.reps):
            s.merge_pairs(h1, h2, *args).free()
        h1.free(); h2.free()
        return None
    routed, (text, qual, lens) = host_route()
    assert routed.download_text() == merged.download_text() and routed.download_quality_text() == merged.download_quality_text(), "the host route merges otherwise"
    routed.free()
    merged_list = [text[i, :lens[i]].tobytes() for i in range(n)]
    best = scan.hamming_best_pattern(pats, merged, 1)
    assert all(np.array_equal(x, y) for x, y in zip(best, scan.hamming_best_pattern(pats, merged_list, 1)))
    n_merged, layout = int((lens > 0).sum()), int(merged.text_bytes)
    merged.free()
    events = Events()
    t = {k: [] for k in ("overlaps", "merge_events", "merge_wall", "host_route", "scan_resident", "scan_host_list")}
    for _ in range(a.reps):
        events.start()
        s.read_overlaps(h1, h2, *args)
        t["overlaps"].append(events.stop_ms())
        events.start()
        merged, ms = wall(lambda: s.merge_pairs(h1, h2, *args))
        t["merge_events"].append(events.stop_ms())
        t["merge_wall"].append(ms)
        (routed, _), ms = wall(host_route)
        t["host_route"].append(ms)
        routed.free()
        t["scan_resident"].append(wall(lambda: scan.hamming_best_pattern(pats, merged, 1))[1])
        t["scan_host_list"].append(wall(lambda: scan.hamming_best_pattern(pats, merged_list, 1))[1])
        merged.free()
    h1.free(); h2.free()
    blocks = (layout - 64) // 64
    in_bytes = int(2 * 2 * READ_LEN * n_merged)  # both reads and both qualities of every merged pair
    write_bytes = in_bytes + 2 * layout + 4 * blocks + (16 + 48) * n
    b, c = statistics.median(t["merge_wall"]), statistics.median(t["host_route"])
    beyond = max(t["merge_wall"]) < min(t["host_route"]) or min(t["merge_wall"]) > max(t["host_route"])
    return {
        "input": {"pairs": n, "read_len": READ_LEN, "fragments": "50..400 uniform", "substitutions": 0.01, "qualities": "33..74 uniform",
                  "min_overlap": a.min_overlap, "max_permille": a.max_permille, "k": 512, "seed": a.seed},
        "result": {"merged": n_merged, "layout_bytes": layout, "merged_bases": int(lens.sum())},
        "ms": {k: summary(v) for k, v in t.items()},
        "merge_over_overlaps": round(statistics.median(t["merge_events"]) / statistics.median(t["overlaps"]), 3),
        "host_route_over_merge": round(c / b, 2), "ranges_apart": bool(beyond),
        "scan_host_list_over_resident": round(statistics.median(t["scan_host_list"]) / statistics.median(t["scan_resident"]), 2),
        "write_bytes": write_bytes, "write_ms_at_peak": round(write_bytes / HBM_PEAK * 1e3, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--min-overlap", type=int, default=10)
    ap.add_argument("--max-permille", type=int, default=200)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--trace-run", action="store_true", help="warm-up and --reps merge calls per size, nothing written: the run a kernel trace wraps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_pairs_bench.json"))
    a = ap.parse_args()
    import sassy_amd
    if sassy_amd.device_count() == 0:
        raise SystemExit("no HIP device visible: nothing is measured without one")
    if a.trace_run:
        for n in a.pairs:
            run_size(sassy_amd, n, a, trace_only=True)
        return 0
    out = {"reps": a.reps, "version": sassy_amd.lib().sassy_hip_version().decode(), "sizes": [run_size(sassy_amd, n, a) for n in a.pairs]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
