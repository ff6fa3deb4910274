"""Records tests/golden/scan_routes.json: the route every row of tests/helpers/scan_routes.py takes on THIS build (the
four route fields of stats() and the number of matches), one fresh Searcher per row.  Run on a device, on the commit whose
routes are to be kept:  python tools/record_scan_routes.py <commit hash> [output path]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import sassy_amd  # noqa: E402
import scan_routes  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "scan_routes.json")
    base = scan_routes.texts()
    rows = scan_routes.rows(base["prose"])
    scan_routes.run_row(sassy_amd, base, rows[0])  # the process's first search loads the kernels
    t0 = time.perf_counter()
    for r in rows:
        r["stats"] = scan_routes.run_row(sassy_amd, base, r)
    seconds = time.perf_counter() - t0
    with open(out, "w") as f:
        f.write('{"recorded_on_commit": %s, "text_bytes": %d, "rows_when_recorded": %d, "replay_seconds_when_recorded": %.2f,\n'
                ' "fields": ["filtered", "piece_len", "fused", "pair", "matches"],\n "rows": [\n'
                % (json.dumps(commit), scan_routes.TEXT_BYTES, len(rows), seconds))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")
    print("recorded", len(rows), "rows in", round(seconds, 2), "s ->", out)


if __name__ == "__main__":
    main()
