"""Deduplication by UMI (DeviceReads.dedup) over seeded synthetic reads -- 150 bases with kept qualities, a 12-base UMI at the 5'
end, Dna, k = 1, `directional` -- with the read batch resident on the device.  The shapes are those of profiles/umi_groups.txt:
dense, 10^6 reads drawn from 10^4 and from 10^3 UMIs with 1 % substitutions per base, and sparse, 10^5 reads of random UMIs.
Run it in a fresh process.

    python tools/bench_dedup_reads.py [--reps 9] [--out profiles/dedup_reads_bench.json]
    python tools/bench_dedup_reads.py --trace-run         # the dedup calls alone, for rocprofv3 --kernel-trace --stats

Per shape, behind a warm-up of every leg whose results are compared -- the columns, the kept reads and both buffers of the new
batch, byte for byte; a difference stops the tool --, the legs in turn, --reps times (median, min, max and (max - min) / median):
  dedup_events      DeviceReads.dedup between two device events
  dedup_wall        the same calls by the host's clock (to set beside the host route)
  groups_wall       DeviceReads.umi_groups alone, by the host's clock
  host_route        what a user did without the call, by the host's clock: the quality buffer and the text downloaded, a numpy
                    gather of the windows, Searcher.umi_groups on them, numpy scores and the best key per group, DeviceReads.select
  encode_bytes      counted, not measured: what dedup_encode_kernel must move -- one 64-byte block read per read, its planes and
                    its table entry written.  The kernels' times come from the kernel trace of a separate run (--trace-run).
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

from tools.bench_merge_pairs import fastq_bytes, wall  # noqa: E402
from tools.bench_read_overlaps import HBM_PEAK, READ_LEN, Events, summary  # noqa: E402

M = 12
SHAPES = [("dense", 1_000_000, 10_000), ("dense", 1_000_000, 1_000), ("sparse", 100_000, 0)]


def synthetic_reads(n: int, n_umis: int, seed: int):
    """(reads, qualities): two (n, 150) uint8 arrays; the first 12 bases one of n_umis UMIs with 1 % substitutions per base
    (n_umis == 0: random)."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = letters[rng.integers(0, 4, (n, READ_LEN))]
    if n_umis:
        umis = letters[rng.integers(0, 4, (n_umis, M))]
        keys = umis[rng.integers(0, n_umis, n)]
        subs = rng.random((n, M)) < 0.01
        reads[:, :M] = np.where(subs, letters[rng.integers(0, 4, (n, M))], keys)
    quals = rng.integers(33, 75, (n, READ_LEN), dtype=np.uint8)
    return np.ascontiguousarray(reads.astype(np.uint8)), np.ascontiguousarray(quals)


def best_per_group(label, score):
    """The kept reads: per label the read of the highest key score << 32 | (0xFFFFFFFF - r), ascending."""
    n = len(label)
    key = (score.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64))
    order = np.lexsort((key, label))
    last = np.flatnonzero(np.append(label[order][1:] != label[order][:-1], True))
    return np.sort(order[last]).astype(np.uint64)


def run_shape(sassy_amd, kind, n, n_umis, a, trace_only=False):
    reads, quals = synthetic_reads(n, n_umis, a.seed + n_umis)
    s = sassy_amd.Searcher("dna", rc=False)
    h = sassy_amd.DeviceReads(fastq_bytes(reads, quals), keep_quality=True)
    call = dict(k=a.k, method="directional")

    def host_route():
        t = np.frombuffer(h.download_text(), dtype=np.uint8)[:n * 192].reshape(n, 192)   # (150 bases: a slot of 192 bytes)
        q = np.frombuffer(h.download_quality_text(), dtype=np.uint8)[:n * 192].reshape(n, 192)[:, :READ_LEN]
        cols = s.umi_groups(np.ascontiguousarray(t[:, :M]), a.k, "directional")
        kept = best_per_group(cols[0], q.sum(axis=1, dtype=np.uint32))
        return h.select(kept), (cols, kept)

    # warm-up of every leg, and the checks
    d = h.dedup(s, M, with_columns=True, **call)
    g = h.umi_groups(s, M, **call)
    if trace_only:  # (the kernels of the dedup alone)
        d.free()
        for _ in range(a.reps):
            h.dedup(s, M, **call).free()
        h.free()
        return None
    routed, (cols, kept) = host_route()
    for name, x, y, z in zip(("label", "size", "rep", "count"), (d.label, d.size, d.rep, d.count), cols, g[:4]):
        if not (np.array_equal(x, y) and np.array_equal(z, y)):
            raise SystemExit(f"{kind} {n}: the device's {name} and the host route's differ")
    if not np.array_equal(d.kept, kept) or (d.n_unique, d.n_groups) != g[4:]:
        raise SystemExit(f"{kind} {n}: the kept reads differ")
    if routed.download_text() != d.reads.download_text() or routed.download_quality_text() != d.reads.download_quality_text():
        raise SystemExit(f"{kind} {n}: the deduplicated batches differ")
    routed.free()
    result = {"n_unique": d.n_unique, "n_groups": d.n_groups, "layout_bytes": int(d.reads.text_bytes)}
    stats = s.stats()
    events = Events()
    t = {k: [] for k in ("dedup_events", "dedup_wall", "groups_wall", "host_route")}
    for _ in range(a.reps):
        d.free()
        events.start()
        d, ms = wall(lambda: h.dedup(s, M, **call))
        t["dedup_events"].append(events.stop_ms())
        t["dedup_wall"].append(ms)
        _, ms = wall(lambda: h.umi_groups(s, M, **call))
        t["groups_wall"].append(ms)
        (routed, _), ms = wall(host_route)
        t["host_route"].append(ms)
        routed.free()
    d.free()
    h.free()
    encode_bytes = n * (64 + 16 + 2 * 4 + 4 + 16)   # the block, the table's start and length, the planes (P W = 2 words), src, flag and number
    b, c = statistics.median(t["dedup_wall"]), statistics.median(t["host_route"])
    beyond = max(t["dedup_wall"]) < min(t["host_route"]) or min(t["dedup_wall"]) > max(t["host_route"])
    return {
        "input": {"shape": kind, "reads": n, "umis": n_umis, "read_len": READ_LEN, "umi_len": M, "substitutions": 0.01 if n_umis else 0.0, "end": "5'",
                  "at": 0, **call, "seed": a.seed + n_umis},
        "result": {**result, "pair_records": int(stats["candidates"]), "relaxation_launches": int(stats["blocks"])},
        "ms": {k: summary(v) for k, v in t.items()},
        "host_route_over_dedup": round(c / b, 2), "ranges_apart": bool(beyond),
        "encode_bytes": encode_bytes, "encode_ms_at_peak": round(encode_bytes / HBM_PEAK * 1e3, 5),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("-k", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--trace-run", action="store_true", help="warm-up and --reps dedup calls per shape, nothing written: the run a kernel trace wraps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_reads_bench.json"))
    a = ap.parse_args()
    import sassy_amd
    if sassy_amd.device_count() == 0:
        raise SystemExit("no HIP device visible: nothing is measured without one")
    if a.trace_run:
        for kind, n, u in SHAPES:
            run_shape(sassy_amd, kind, n, u, a, trace_only=True)
        return 0
    out = {"reps": a.reps, "version": sassy_amd.lib().sassy_hip_version().decode(), "shapes": [run_shape(sassy_amd, kind, n, u, a) for kind, n, u in SHAPES]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
