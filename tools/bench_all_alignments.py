"""search_all (traced) against search_all_alignments on three inputs (DESIGN.md "search_all_alignments"):

  (a) config 2's shape: a 3 GB device-resident random-DNA text, m = 32, k = 3, one plant per MiB, both strands;
  (b) the reference's perf.rs shape: 100 kB of random DNA, m = 23, k = 3 (host text);
  (c) a low-complexity text (microsatellite-like repeats with point changes), m = 32, k = 6.

Per input: the median wall time of each call, the split of search_all_alignments into its search and its enumeration
launches (HIP events: stats scan_ms / trace_ms), end positions, alignments and alignments per second.  One JSON line
per input, and all of them into --out.

    python tools/bench_all_alignments.py [--text-bytes 3000000000] [--reps 5] [--only a,b,c] [--out profiles/x.json]
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
import sassy_amd  # noqa: E402


class DevText:
    """A device-resident text as the Python surface reads a tensor (data_ptr, numel, is_cuda, a 1-byte dtype)."""

    class _Byte:
        itemsize = 1

    dtype = _Byte()
    is_cuda = True

    def __init__(self, ptr: int, n: int):
        self._p, self._n = ptr, n

    def data_ptr(self):
        return self._p

    def numel(self):
        return self._n

    def is_contiguous(self):
        return True


def _timed(f, reps):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def run(name, s, pat, text, k, reps, n_bytes):
    s.set_timing(2)
    f_all = lambda: s.search_all(pat, text, k)  # noqa: E731
    f_all()
    t_all, ms = _timed(f_all, reps)
    st_all = s.stats()
    f_aa = lambda: s.search_all_alignments(pat, text, k)  # noqa: E731
    f_aa()
    t_aa, groups = _timed(f_aa, reps)
    st = s.stats()
    n_aln = sum(len(g) for g in groups)
    row = {
        "input": name, "text_bytes": n_bytes, "m": len(pat), "k": k, "strands": 2,
        "search_all_ms": round(t_all, 3), "search_all_trace_ms": round(st_all["trace_ms"], 3),
        "all_alignments_ms": round(t_aa, 3), "ratio": round(t_aa / t_all, 3),
        "aa_search_scan_ms": round(st["scan_ms"], 3), "aa_enumerate_ms": round(st["trace_ms"], 3),
        "aa_total_ms": round(st["total_ms"], 3),
        "ends": int(st["candidates"]), "search_all_matches": len(ms), "groups": len(groups), "alignments": n_aln,
        "alignments_per_s": round(n_aln / (t_aa / 1e3), 1),
    }
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-bytes", type=int, default=3_000_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = random.Random(23)
    rows = []
    want = set(args.only.split(","))
    if "a" in want:
        n = args.text_bytes
        buf = sassy_amd.DeviceBuffer(n + 4096)
        sassy_amd.generate_dna(buf.ptr, n, 42, 0)
        pat = bytes(rng.choice(b"ACGT") for _ in range(32))
        planted = sassy_amd.plant(buf.ptr, n, 0, n, 42, pat, 3, stride=1 << 20)
        s = sassy_amd.Searcher("dna", rc=True)
        s.text_unchanged(True)
        row = run("a_3GB_m32_k3", s, pat, DevText(buf.ptr, n), 3, args.reps, n)
        row["planted"] = planted
        rows.append(row)
        del buf
    if "b" in want:
        text = bytes(rng.choice(b"ACGT") for _ in range(100_000))
        pat = bytes(rng.choice(b"ACGT") for _ in range(23))
        rows.append(run("b_100kB_m23_k3", sassy_amd.Searcher("dna", rc=True), pat, text, 3, args.reps, len(text)))
    if "c" in want:
        units = [b"AC", b"AAT", b"AGGC", b"A"]
        t = bytearray()
        while len(t) < 1_000_000:
            t += rng.choice(units) * rng.randint(20, 200)
            t += bytes(rng.choice(b"ACGT") for _ in range(rng.randint(50, 400)))
        for _ in range(len(t) // 50):  # point changes inside the repeats
            t[rng.randrange(len(t))] = rng.choice(b"ACGT")
        text = bytes(t[:1_000_000])
        pat = b"ACACACACACACACACACACACACACACACAC"
        rows.append(run("c_lowcomplexity_1MB_m32_k6", sassy_amd.Searcher("dna", rc=True), pat, text, 6, args.reps,
                        len(text)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
