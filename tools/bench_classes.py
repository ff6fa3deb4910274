"""What a character-class pattern costs next to a literal one: three searches at the same m and k over one device-resident
text of prose, all on the streaming DP.

    python tools/bench_classes.py [--text-bytes 1000000000] [--reps 10] [--out profiles/classes_bench.json]

  literal    a literal pattern through Searcher("ascii").set_prefilter(0): the streaming DP as every Ascii search without
             a prefilter runs it
  singleton  the same pattern as singleton classes (search_classes): the same slots, one cube each
  classes    a realistic class pattern of the same length: digit and letter ranges, a complement, literals

Per run: scan_ms = the HIP-event time of the scan kernel (median over the repetitions), wall_ms = the mean wall time of a
search.  The file records both and the ratios to the literal run.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LITERAL = b"kernel timeout 2026-10-17 dev"                        # m = 29
CLASSES = rb"[Kk]ernel [a-z][a-z][a-z][a-z][a-z][a-z][a-z] \d\d\d\d-\d\d-\d\d [^ ]ev"  # m = 29


def main():
    import sassy_amd
    from helpers.prose_text import DevText, prose
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-bytes", type=float, default=1e9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("-k", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classes_bench.json"))
    a = ap.parse_args()
    n = int(a.text_bytes) // 64 * 64
    rng = random.Random(1)
    piece = bytearray(prose(rng, 1 << 20))
    piece[5000:5000 + len(LITERAL)] = LITERAL  # one exact occurrence per MiB
    piece = bytes(piece)
    buf = sassy_amd.DeviceBuffer(n + 4096)
    for off in range(0, n, len(piece)):
        buf.upload(piece[:min(len(piece), n - off)], off)
    dev = DevText(buf.ptr, n)
    cls = sassy_amd.parse_classes(CLASSES)
    single = sassy_amd.ClassPattern.from_sets([[c] for c in LITERAL])
    assert cls.m == single.m == len(LITERAL)
    s = sassy_amd.Searcher("ascii", rc=False)
    s.set_prefilter(0)
    s.text_unchanged(True)
    runs = {
        "literal": lambda: s.search(LITERAL, dev, a.k),
        "singleton": lambda: s.search_classes(single, dev, a.k),
        "classes": lambda: s.search_classes(cls, dev, a.k),
    }
    def cubes(p):  # all distinct sets of the pattern together
        distinct = {frozenset(p.members(j)) for j in range(p.m)}
        return sum(len(sassy_amd.class_cover(x)[0]) for x in distinct)

    out = {"text_bytes": n, "m": len(LITERAL), "k": a.k, "reps": a.reps, "literal": LITERAL.decode(), "class_expression": CLASSES.decode(),
           "cubes": {"singleton": cubes(single), "classes": cubes(cls)}, "runs": {}}
    for name, fn in runs.items():
        for _ in range(3):
            r = fn()
        scan = []
        t0 = time.perf_counter()
        for _ in range(a.reps):
            r = fn()
            scan.append(s.stats()["scan_ms"])
        wall = (time.perf_counter() - t0) / a.reps * 1e3
        out["runs"][name] = {"scan_ms": round(statistics.median(scan), 4), "wall_ms": round(wall, 4), "matches": len(r),
                             "GB_per_s": round(n / statistics.median(scan) / 1e6, 1)}
        print(name, out["runs"][name], flush=True)
    lit = out["runs"]["literal"]["scan_ms"]
    out["scan_ratio_to_literal"] = {k: round(v["scan_ms"] / lit, 3) for k, v in out["runs"].items()}
    assert out["runs"]["singleton"]["matches"] == out["runs"]["literal"]["matches"], "singleton classes must find what the literal finds"
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out["scan_ratio_to_literal"]))
    buf.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
