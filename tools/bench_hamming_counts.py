"""hamming_counts next to the record path it replaces, over the same device-resident text: device-generated DNA, both calls
alternated inside one repetition loop so that they see the same machine.  Run it in a fresh process.

    python tools/bench_hamming_counts.py [--text-bytes 1000000000] [--reps 7] [--out profiles/hamming_counts_bench.json]

  counts    Searcher.hamming_counts(patterns, text, k)
  records   Searcher.search_hamming(patterns, text, k, without_trace=True, as_result=True) -- the yardstick: what a caller had
            to do before, less the count on the host

Cases: (m, k) = (23, 3) and (20, 4) with 1 and with 16 patterns, both strands, on random DNA (hits are sparse); and a dense
case: the same text with 16 stretches of 1 MiB of A planted, one pattern of 23 A at k = 3 (every start of a stretch is a hit).
Per run and call: call_ms = the call's wall time (stats total_ms), scan_ms = the HIP-event time of the scan launches -- median,
min, max and (max - min) / median over the repetitions -- and the record path's number of scan launches (more than the
pattern groups: item ranges were cut and launched again).  The file records counts / records of the medians.
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((23, 3), (20, 4))
STRETCH = 1 << 20
N_STRETCHES = 16


def summary(v):
    med = statistics.median(v)
    return {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4), "spread": round((max(v) - min(v)) / med, 4) if med else 0.0}


def run_case(sassy_amd, dev, n, pats, k, reps):
    import numpy as np
    cnt = sassy_amd.Searcher("dna", rc=True)
    rec = sassy_amd.Searcher("dna", rc=True)
    runs = {
        "counts": (cnt, lambda: cnt.hamming_counts(pats, dev, k)),
        "records": (rec, lambda: rec.search_hamming(pats, dev, k, without_trace=True, as_result=True)),
    }
    for _, fn in runs.values():  # warm-up: code objects, buffers
        for _ in range(2):
            fn()
    call = {name: [] for name in runs}
    scan = {name: [] for name in runs}
    info = {}
    for _ in range(reps):  # alternated: every repetition runs both
        for name, (s, fn) in runs.items():
            r = fn()
            st = s.stats()
            call[name].append(st["total_ms"])
            scan[name].append(st["scan_ms"])
            info[name] = {"hits": int(st["candidates"]), "scan_launches": int(st["scan_launches"])}
            if name == "counts":
                table = r
            else:
                arr = r.array
                bins = (2 * arr["pattern_idx"].astype(np.int64) + arr["strand"]) * (k + 1) + arr["cost"]
                want = np.bincount(bins, minlength=table.size).reshape(table.shape)
                del r, arr
    out = {"m": len(pats[0]), "k": k, "patterns": len(pats), "strands": 2, "tables_agree": bool(np.array_equal(table, want)), "runs": {}}
    for name in runs:
        out["runs"][name] = {"call_ms": summary(call[name]), "scan_ms": summary(scan[name]), **info[name],
                             "GB_per_s_call": round(n / statistics.median(call[name]) / 1e6, 1)}
    out["counts_over_records_call"] = round(out["runs"]["counts"]["call_ms"]["median"] / out["runs"]["records"]["call_ms"]["median"], 4)
    out["counts_over_records_scan"] = round(out["runs"]["counts"]["scan_ms"]["median"] / out["runs"]["records"]["scan_ms"]["median"], 4)
    print(json.dumps(out), flush=True)
    return out


def main():
    import sassy_amd
    from helpers.prose_text import DevText
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-bytes", type=float, default=1e9)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dense-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hamming_counts_bench.json"))
    a = ap.parse_args()
    n = int(a.text_bytes) // 64 * 64
    buf = sassy_amd.DeviceBuffer(n + 4096)
    sassy_amd.generate_dna(buf.ptr, n, 20261019)
    dev = DevText(buf.ptr, n)
    rng = random.Random(1)
    out = {"text_bytes": n, "reps": a.reps, "dense_reps": a.dense_reps,
           "text": "generate_dna(seed 20261019), one exact copy of pattern 0 per 64 MiB; dense: plus 16 stretches of 1 MiB of A", "sparse": [], "dense": []}
    for m, k in SHAPES:
        pats = [bytes(rng.choice(b"ACGT") for _ in range(m)) for _ in range(16)]
        for off in range(1 << 20, n - m, 64 << 20):
            buf.upload(pats[0], off + 37)
        for np_ in (1, 16):
            out["sparse"].append(run_case(sassy_amd, dev, n, pats[:np_], k, a.reps))
    stretch = b"A" * STRETCH
    step = max(STRETCH, (n - STRETCH) // N_STRETCHES // 64 * 64)
    planted = 0
    for i in range(N_STRETCHES):
        if i * step + STRETCH <= n:
            buf.upload(stretch, i * step)
            planted += 1
    out["dense_stretches"] = planted
    out["dense"].append(run_case(sassy_amd, dev, n, [b"A" * 23], 3, a.dense_reps))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    buf.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
