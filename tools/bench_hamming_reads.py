"""Demultiplexing-shaped Hamming search over a batch of reads: host-generated reads with planted barcodes, five legs
alternated inside one repetition loop so that they see the same machine.

    python tools/bench_hamming_reads.py [--reads 100000] [--reps 7] [--out profiles/hamming_many_bench.json]

  per_record     the shape before the batch calls: one Searcher.search_hamming call per read (on the first --loop-reads
                 reads, reported per read)
  many           Searcher.search_hamming_many over all reads (without trace)
  best           Searcher.hamming_best_pattern over all reads
  edit_best      Searcher.best_pattern (edit distance) on the same inputs
  layout_upload  the batch call's layout, upload and rem table alone: a search_hamming_many call whose only pattern is
                 longer than every read, so that no scan is launched

100 000 reads of 150 bp, 96 barcodes of 16-24 bp planted with 0-2 substitutions on either strand, k = 2, Dna, both strands.
Times are wall-clock milliseconds of the whole call (median, min and max over the repetitions); the file records the
per-read times, the ratio of every batch leg to per_record and the run-to-run spread of every leg.
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

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def make_inputs(n_reads, read_len, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    barcodes = [letters[rng.integers(0, 4, int(rng.integers(16, 25)))].tobytes() for _ in range(96)]
    reads = letters[rng.integers(0, 4, (n_reads, read_len))]
    which = rng.integers(0, 96, n_reads)
    for i in range(n_reads):
        bc = barcodes[which[i]]
        if rng.integers(0, 2):
            bc = bc.translate(COMP)[::-1]
        w = np.frombuffer(bc, dtype=np.uint8).copy()
        for _ in range(int(rng.integers(0, 3))):
            w[rng.integers(0, len(w))] = letters[rng.integers(0, 4)]
        at = int(rng.integers(0, read_len - len(w) + 1))
        reads[i, at:at + len(w)] = w
    return barcodes, [row.tobytes() for row in reads]


def main():
    import sassy_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--loop-reads", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("-k", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hamming_many_bench.json"))
    a = ap.parse_args()
    barcodes, reads = make_inputs(a.reads, a.read_len, 20261019)
    batch = sassy_amd.TextBatch.from_list(reads)
    head = reads[:min(a.loop_reads, len(reads))]
    s = sassy_amd.Searcher("dna", rc=True)
    too_long = [b"A" * 1024]
    found = {}

    def per_record():
        n = 0
        for r in head:
            n += len(s.search_hamming(barcodes, r, a.k, without_trace=True, as_result=True).array)
        found["per_record"] = n

    def many():
        found["many"] = len(s.search_hamming_many(barcodes, batch, a.k, without_trace=True, as_result=True).array)

    def best():
        found["best"] = int((s.hamming_best_pattern(barcodes, batch, a.k)[0] != sassy_amd.NO_MATCH).sum())

    def edit_best():
        found["edit_best"] = int((s.best_pattern(barcodes, batch, a.k)[0] != sassy_amd.NO_MATCH).sum())

    def layout_upload():
        found["layout_upload"] = len(s.search_hamming_many(too_long, batch, a.k, without_trace=True, as_result=True).array)

    legs = {"per_record": (per_record, len(head)), "many": (many, len(reads)), "best": (best, len(reads)),
            "edit_best": (edit_best, len(reads)), "layout_upload": (layout_upload, len(reads))}
    times = {name: [] for name in legs}
    scan_ms = {}
    for name, (fn, _) in legs.items():  # warm-up: code objects, buffers
        fn()
    for _ in range(a.reps):  # alternated: every repetition runs all five
        for name, (fn, _) in legs.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
            scan_ms[name] = s.stats()["scan_ms"]
    out = {"reads": len(reads), "read_len": a.read_len, "barcodes": len(barcodes), "k": a.k, "reps": a.reps, "loop_reads": len(head),
           "bytes_laid_out": len(reads) * ((a.read_len + 63) // 64 * 64), "legs": {}}
    for name, v in times.items():
        med, n = statistics.median(v), legs[name][1]
        out["legs"][name] = {"ms": round(med, 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                             "spread": round((max(v) - min(v)) / med, 4), "us_per_read": round(med * 1e3 / n, 4),
                             "last_scan_ms": round(scan_ms[name], 4), "found": found[name]}
        print(name, out["legs"][name], flush=True)
    base = out["legs"]["per_record"]["us_per_read"]
    out["per_read_ratio_to_per_record"] = {name: round(v["us_per_read"] / base, 5) for name, v in out["legs"].items()}
    print(json.dumps(out["per_read_ratio_to_per_record"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
