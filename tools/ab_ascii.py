"""A/B of the case-sensitive `ascii` search between two builds of the library on one box (SASSY_HIP_LIBRARY, the A/B switch
of sassy_amd/__init__.py): a lone search, m = 32, k = 3, on the synthetic device-resident text (bench.py's generator, one
plant per MiB), the streaming DP that every Ascii search takes.

    python tools/ab_ascii.py --parent path/to/parent/libsassy_hip.so [--runs 5] [--text-bytes 3000000000] [--out profiles/ascii_ci_ab.txt]

Every run is a fresh process (its own text, warm-up, 20 timed searches: the mean wall time per search); the two builds
alternate.  The new build passes when its median lies inside the parent's own run-to-run spread (min .. max) or below it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_run(n, m, k):
    import sassy_amd
    from bench import _dna_bytes
    pat = bytes(_dna_bytes(43, 0, m))
    buf = sassy_amd.DeviceBuffer(n + 4096)
    sassy_amd.generate_dna(buf.ptr, n, 42, 0)
    sassy_amd.plant(buf.ptr, n, 0, n, 42, pat, k, 1 << 20)
    s = sassy_amd.Searcher("ascii", rc=False)
    for _ in range(5):
        r = s.search_shard(pat, buf.ptr, 0, n, 0, n, k)
    kernel = s.stats()["scan_ms"]
    s.set_timing(0)
    for _ in range(3):
        s.search_shard(pat, buf.ptr, 0, n, 0, n, k)
    t0 = time.perf_counter()
    for _ in range(20):
        s.search_shard(pat, buf.ptr, 0, n, 0, n, k)
    ms = (time.perf_counter() - t0) / 20 * 1e3
    print(json.dumps({"lone_ms": round(ms, 4), "scan_ms": round(kernel, 4), "matches": len(r), "library": sassy_amd.library_path()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--text-bytes", type=float, default=3e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ascii_ci_ab.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    n = int(a.text_bytes) // 64 * 64
    if a.child:
        return one_run(n, 32, 3)
    if not a.parent or not os.path.exists(a.parent):
        raise SystemExit("--parent: the parent build's libsassy_hip.so")
    res = {"parent": [], "new": []}
    lines = [f"ascii (case-sensitive), m = 32, k = 3, lone search on a {n} byte device-resident synthetic text, one plant per MiB",
             "per run: a fresh process, mean wall ms per search over 20 searches (scan_ms: HIP events of one search's scan)"]
    for i in range(a.runs):
        for which in ("parent", "new"):
            env = dict(os.environ)
            env.pop("SASSY_HIP_LIBRARY", None)
            if which == "parent":
                env["SASSY_HIP_LIBRARY"] = os.path.abspath(a.parent)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--text-bytes", str(n)], env=env,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"{which} run {i} failed ({p.returncode}): {p.stderr[-2000:]}")
            d = json.loads(p.stdout.strip().splitlines()[-1])
            res[which].append(d)
            lines.append(f"run {i} {which:6s} lone_ms {d['lone_ms']:.4f} scan_ms {d['scan_ms']:.4f} matches {d['matches']}")
            print(lines[-1], flush=True)
    if {d["matches"] for d in res["parent"]} != {d["matches"] for d in res["new"]}:
        raise SystemExit("the two builds disagree on the number of matches")
    pm, nm = [d["lone_ms"] for d in res["parent"]], [d["lone_ms"] for d in res["new"]]
    verdict = "PASS" if statistics.median(nm) <= max(pm) else "FAIL"
    lines.append(f"parent: median {statistics.median(pm):.4f} ms, spread {min(pm):.4f} .. {max(pm):.4f}")
    lines.append(f"new:    median {statistics.median(nm):.4f} ms, spread {min(nm):.4f} .. {max(nm):.4f}")
    lines.append(f"{verdict}: the new build's median {'lies inside or below' if verdict == 'PASS' else 'lies above'} the parent's run-to-run spread")
    print("\n".join(lines[-3:]), flush=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0 if verdict == "PASS" else 1


if __name__ == "__main__":
    sys.exit(main())
