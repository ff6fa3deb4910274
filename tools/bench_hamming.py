"""The Hamming scan next to the DP over the same device-resident text: device-generated DNA, four runs per (m, k),
alternated inside one repetition loop so that they see the same machine.

    python tools/bench_hamming.py [--text-bytes 1000000000] [--reps 9] [--out profiles/hamming_bench.json]

  hamming_1    Searcher.search_hamming with one pattern (without trace)
  hamming_16   ... with 16 patterns of the same length in one call: one pass over the text
  dp_streaming the forced streaming DP: set_prefilter(0), search_all without trace -- the yardstick
  dp_filtered  the default search_all without trace (the prefilter the library chooses)

Per run: scan_ms = the HIP-event time of the scan path (median, min and max over the repetitions), GB/s = text bytes over
the median.  The file records the ratios of the medians to dp_streaming and the run-to-run spread of every run.
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

SHAPES = ((32, 3), (23, 3))


def main():
    import sassy_amd
    from helpers.prose_text import DevText
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-bytes", type=float, default=1e9)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hamming_bench.json"))
    a = ap.parse_args()
    n = int(a.text_bytes) // 64 * 64
    buf = sassy_amd.DeviceBuffer(n + 4096)
    sassy_amd.generate_dna(buf.ptr, n, 20261018)
    dev = DevText(buf.ptr, n)
    rng = random.Random(1)
    out = {"text_bytes": n, "reps": a.reps, "text": "generate_dna(seed 20261018), one exact copy of pattern 0 per 64 MiB", "shapes": []}
    flags = sassy_amd.ALL_MINIMA | sassy_amd.WITHOUT_TRACE
    for m, k in SHAPES:
        pats = [bytes(rng.choice(b"ACGT") for _ in range(m)) for _ in range(16)]
        for off in range(1 << 20, n - m, 64 << 20):
            buf.upload(pats[0], off + 37)
        ham = sassy_amd.Searcher("dna", rc=False)
        dp = sassy_amd.Searcher("dna", rc=False).set_prefilter(0)
        flt = sassy_amd.Searcher("dna", rc=False)
        for s in (ham, dp, flt):
            s.text_unchanged(True)
        runs = {
            "hamming_1": (ham, lambda: ham.search_hamming(pats[0], dev, k, without_trace=True, as_result=True)),
            "hamming_16": (ham, lambda: ham.search_hamming(pats, dev, k, without_trace=True, as_result=True)),
            "dp_streaming": (dp, lambda: dp._search(pats[0], dev, k, flags)),
            "dp_filtered": (flt, lambda: flt._search(pats[0], dev, k, flags)),
        }
        scan = {name: [] for name in runs}
        found = {}
        kinds = {}
        for name, (s, fn) in runs.items():  # warm-up: code objects, buffers
            for _ in range(2):
                fn()
        for _ in range(a.reps):  # alternated: every repetition runs all four
            for name, (s, fn) in runs.items():
                r = fn()
                st = s.stats()
                scan[name].append(st["scan_ms"])
                found[name] = len(r.array)
                kinds[name] = st["filtered"]
        shape = {"m": m, "k": k, "runs": {}}
        for name, v in scan.items():
            med = statistics.median(v)  # (0 where the run's route records no scan_ms: no spread, no rate)
            shape["runs"][name] = {"scan_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                                   "spread": round((max(v) - min(v)) / med, 4) if med else None,
                                   "GB_per_s": round(n / med / 1e6, 1) if med else None,
                                   "records": found[name], "filtered": kinds[name]}
            print(m, k, name, shape["runs"][name], flush=True)
        base = shape["runs"]["dp_streaming"]["scan_ms"]
        shape["ratio_to_dp_streaming"] = {name: round(v["scan_ms"] / base, 4) for name, v in shape["runs"].items()}
        shape["hamming_16_per_pattern_ms"] = round(shape["runs"]["hamming_16"]["scan_ms"] / 16, 4)
        out["shapes"].append(shape)
        print(json.dumps(shape["ratio_to_dp_streaming"]), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    buf.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
