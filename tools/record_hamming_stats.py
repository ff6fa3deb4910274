"""Records tests/golden/hamming_stats.json: the stats() of every call of tests/helpers/hamming_stats.py on THIS build (all
fields but the times, and the number of records), one fresh Searcher per call.  Run on a device, on the commit whose
counters are to be kept:  python tools/record_hamming_stats.py <commit hash> [output path]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import sassy_amd  # noqa: E402
import hamming_stats  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "hamming_stats.json")
    base = hamming_stats.texts()
    calls = hamming_stats.calls()
    hamming_stats.run_call(sassy_amd, base, calls[0])  # the process's first search loads the kernels
    t0 = time.perf_counter()
    for c in calls:
        c["stats"] = hamming_stats.run_call(sassy_amd, base, c)
    seconds = time.perf_counter() - t0
    with open(out, "w") as f:
        f.write('{"recorded_on_commit": %s, "text_bytes": %d, "calls_when_recorded": %d, "replay_seconds_when_recorded": %.2f,\n "calls": [\n'
                % (json.dumps(commit), hamming_stats.TEXT_BYTES, len(calls), seconds))
        f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in calls))
        f.write("\n]}\n")
    print("recorded", len(calls), "calls in", round(seconds, 2), "s ->", out)


if __name__ == "__main__":
    main()
