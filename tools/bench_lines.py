"""Line resolution on the device (sassy_amd/csrc/line_index.hip): the index pass and the resolve pass, timed
apart by HIP events, on a synthetic device-resident text -- printable bytes with a newline planted every ~80 bytes, and the
same text without any newline (one line: every line start / end is found through the index's "none" answers) -- for 10^3
and 10^6 spans.  Next to it the lone case-sensitive `ascii` search (m = 32, k = 3) of the same text on the same box.

    python tools/bench_lines.py [--text-bytes 3000000000] [--reps 5] [--out profiles/line_spans_bench.json]

Prints one JSON line per case (GB/s of the index pass and its fraction of the 8 TB/s peak) and writes all of them to --out.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sassy_amd  # noqa: E402
from tools.bench_all_alignments import DevText  # noqa: E402

PEAK_GBS = 8000.0


def make_text(n, with_newlines, chunk=1 << 26):
    """n printable bytes on the device, uploaded chunk by chunk; with_newlines: one '\\n' in every 80 bytes, at a place
    that moves from line to line."""
    buf = sassy_amd.DeviceBuffer(n + 4096)
    rng = np.random.default_rng(1)
    block = rng.integers(32, 127, size=chunk, dtype=np.uint8)
    if with_newlines:
        at = np.arange(0, chunk, 80) + rng.integers(0, 80, size=(chunk + 79) // 80)
        block[at[at < chunk]] = 10
    for off in range(0, n, chunk):
        part = block[:min(chunk, n - off)]
        buf.upload(part.tobytes(), off)
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-bytes", type=float, default=3e9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_spans_bench.json"))
    a = ap.parse_args()
    n = int(a.text_bytes) // 64 * 64
    s = sassy_amd.Searcher("ascii", rc=False)
    s.set_timing(2)
    L = sassy_amd.lib()
    rows = []
    rng = np.random.default_rng(2)
    for name, with_nl in (("newline every ~80 bytes", True), ("no newline", False)):
        buf = make_text(n, with_nl)
        dev = DevText(buf.ptr, n)
        for count in (1000, 1_000_000):
            first = rng.integers(0, n, size=count, dtype=np.uint64)
            last = np.minimum(first + rng.integers(0, 40, size=count, dtype=np.uint64), n).astype(np.uint64)
            s.line_spans(dev, first, last)  # warm-up: allocations
            idx, res, wall = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                spans = s.line_spans(dev, first, last)
                wall.append((time.perf_counter() - t0) * 1e3)
                i_ms, r_ms = C.c_double(), C.c_double()
                L.sassy_hip_line_span_times(s._h, C.byref(i_ms), C.byref(r_ms))
                idx.append(i_ms.value)
                res.append(r_ms.value)
            i_med, r_med = statistics.median(idx), statistics.median(res)
            row = {"text": name, "text_bytes": n, "spans": count, "index_ms": round(i_med, 4), "resolve_ms": round(r_med, 4),
                   "wall_ms": round(statistics.median(wall), 4), "index_GBs": round(n / i_med / 1e6, 1),
                   "index_frac_of_peak": round(n / i_med / 1e6 / PEAK_GBS, 4), "resolve_ns_per_span": round(r_med * 1e6 / count, 2),
                   "lines": int(spans["line_no"].max())}
            rows.append(row)
            print(json.dumps(row), flush=True)
        if with_nl:  # the lone ascii search of the same text, for scale
            pat = bytes(rng.integers(97, 123, size=32, dtype=np.uint8))
            for _ in range(3):
                s.search_shard(pat, buf.ptr, 0, n, 0, n, 3)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                s.search_shard(pat, buf.ptr, 0, n, 0, n, 3)
                ts.append((time.perf_counter() - t0) * 1e3)
            row = {"text": name, "text_bytes": n, "lone_ascii_search_ms": round(statistics.median(ts), 4), "m": 32, "k": 3,
                   "scan_ms": round(s.stats()["scan_ms"], 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        buf.free()
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
