"""Adapter and quality trimming (Searcher.trim_reads) over seeded synthetic reads -- 150 bases cut from fragments of 30 .. 250
bases as in tools/bench_read_overlaps.py, the adapter and random bases behind a fragment shorter than the read, 1 %
substitutions, Dna, qualities that decay toward the 3' end -- with the read batch resident on the device.  Run it in a fresh
process.

    python tools/bench_trim_reads.py [--reads 100000 1000000] [--reps 9] [--out profiles/trim_reads_bench.json]
    python tools/bench_trim_reads.py --trace-run          # the trim calls alone, for rocprofv3 --kernel-trace --stats

Per size, behind a warm-up of every leg whose trimmed reads are checked on a sample against tests/helpers/trim_reads_ref.py,
the legs in turn, --reps times (median, min, max and (max - min) / median each):
  trim          Searcher.trim_reads: between two device events, and by the host's clock as well (to set beside the host route)
  host_route    what a user did without the call, by the host's clock: the text and the quality buffer downloaded, a numpy
                trim over all reads at once, the trimmed reads as FASTQ bytes, DeviceReads of them with kept qualities
  scan_trimmed  hamming_best_pattern (16 patterns of 12 bases, k = 1) on the trimmed handle, and the same call on the host
                list of the trimmed reads, by the host's clock: the batch is used in place
  find_bound    counted, not measured: the rounds of positions the find kernel walks (a read's walk ends with the round that
                accepts a position) and the vector instructions they issue, against the machine's issue rate
  write_bytes   counted, not measured: what reads_window_write_kernel must move.  The kernels' times come from the kernel trace
                of a separate run (--trace-run).
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

from tools.bench_merge_pairs import fastq_bytes, merged_fastq, wall  # noqa: E402
from tools.bench_read_overlaps import CLOCK_HZ, HBM_PEAK, READ_LEN, SIMDS, VALU_ISSUE_CYCLES, Events, summary  # noqa: E402

ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
# v_* instructions of trim_find_kernel<6, false> per round of 64 positions: the three-word windows of three planes, and per
# adapter the mismatch words, popcounts, acceptance and combine (gfx950, -O3; read off the unit's disassembly)
VALU_PER_ROUND = 16
VALU_PER_ROUND_AND_ADAPTER = 35


def synthetic_reads(n: int, seed: int):
    """(reads, qualities, fragment lengths): two (n, 150) uint8 arrays."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = letters[rng.integers(0, 4, (n, READ_LEN))]
    frag = rng.integers(30, 251, n)
    ad = np.frombuffer(ADAPTER, dtype=np.uint8)
    col = np.arange(READ_LEN)[None, :]
    j = col - frag[:, None]
    in_ad = (j >= 0) & (j < len(ad))
    reads = np.where(in_ad, ad[np.clip(j, 0, len(ad) - 1)], reads)
    subs = rng.random((n, READ_LEN)) < 0.01
    reads = np.where(subs, letters[rng.integers(0, 4, (n, READ_LEN))], reads).astype(np.uint8)
    quals = np.clip(33 + 38 - col * 26 // READ_LEN + rng.integers(-10, 11, (n, READ_LEN)), 33, 74).astype(np.uint8)
    return np.ascontiguousarray(reads), np.ascontiguousarray(quals), frag


def numpy_trim(reads, quals, a):
    """The definition over (n, 150) arrays, one adapter: (lengths, found)."""
    n, L = reads.shape
    lq = np.full(n, L, dtype=np.int64)
    if a.quality_cutoff:
        terms = quals.astype(np.int32) - 33 - a.quality_cutoff
        s = np.cumsum(terms[:, ::-1], axis=1)[:, ::-1]
        col = np.arange(L)[None, :]
        stop = np.where(s > 0, col, -1).max(axis=1)
        seen = col > stop[:, None]
        low = np.where(seen, s, 1 << 30)
        mn = low.min(axis=1)
        at = np.where(seen & (s == mn[:, None]), col, -1).max(axis=1)
        lq = np.where(mn < 0, at, L).astype(np.int64)
    ad = np.frombuffer(ADAPTER, dtype=np.uint8)
    m = len(ad)
    padded = np.zeros((n, L + m), dtype=np.uint8)
    padded[:, :L] = reads
    col = np.arange(L)[None, :]
    mm = np.zeros((n, L), dtype=np.uint8)  # (at most 33 a cell)
    left = (lq[:, None] - col).astype(np.int16)  # rows of the read from c on, in front of lq
    for i in range(m):
        mm += (padded[:, i:i + L] != ad[i]) & (left > i)
    ov = np.minimum(m, left)
    ok = (ov >= a.min_overlap) & (mm.astype(np.int32) * 1000 <= a.max_permille * ov.astype(np.int32))
    found = ok.any(axis=1)
    cut = np.where(found, ok.argmax(axis=1), lq)
    return np.where(cut >= a.min_length, cut, 0).astype(np.int64), found


def run_size(sassy_amd, n, a, trace_only=False):
    import trim_reads_ref as tref
    reads, quals, frag = synthetic_reads(n, a.seed)
    s = sassy_amd.Searcher("dna", rc=False)
    scan = sassy_amd.Searcher("dna", rc=True)
    h = sassy_amd.DeviceReads(fastq_bytes(reads, quals), keep_quality=True)
    call = dict(min_overlap=a.min_overlap, k=512, max_permille=a.max_permille, quality_cutoff=a.quality_cutoff, min_length=a.min_length)
    pats = [bytes(np.random.default_rng(7 + i).choice(np.frombuffer(b"ACGT", dtype=np.uint8), 12).astype(np.uint8)) for i in range(16)]

    def host_route():
        t = np.frombuffer(h.download_text(), dtype=np.uint8)[:n * 192].reshape(n, 192)[:, :READ_LEN]  # (150 bases: a slot of 192 bytes)
        q = np.frombuffer(h.download_quality_text(), dtype=np.uint8)[:n * 192].reshape(n, 192)[:, :READ_LEN]
        lens, found = numpy_trim(t, q, a)
        return sassy_amd.DeviceReads(merged_fastq(t, q, lens), keep_quality=True), (t, lens, found)

    # warm-up of every leg, and the check on a sample
    trimmed, rec = s.trim_reads(h, [ADAPTER], with_records=True, **call)
    sample = np.random.default_rng(1).choice(n, 300, replace=False).tolist()
    want = tref.expected_trim("dna", [(reads[i].tobytes(), quals[i].tobytes()) for i in sample], [ADAPTER], **call)
    assert np.array_equal(rec[sample], want[0]), "the call's records and the definition disagree"
    assert [trimmed.download(i) for i in sample] == want[1] and [trimmed.quality(i) for i in sample] == want[2], "the trim and the definition disagree"
    if trace_only:  # (the kernels of the trim alone)
        trimmed.free()
        for _ in range(a.reps):
            s.trim_reads(h, [ADAPTER], **call).free()
        h.free()
        return None
    routed, (text, lens, found) = host_route()
    assert routed.download_text() == trimmed.download_text() and routed.download_quality_text() == trimmed.download_quality_text(), "the host route trims otherwise"
    routed.free()
    trimmed_list = [text[i, :lens[i]].tobytes() for i in range(n)]
    best = scan.hamming_best_pattern(pats, trimmed, 1)
    assert all(np.array_equal(x, y) for x, y in zip(best, scan.hamming_best_pattern(pats, trimmed_list, 1)))
    layout = int(trimmed.text_bytes)
    trimmed.free()
    events = Events()
    t = {k: [] for k in ("trim_events", "trim_wall", "host_route", "scan_resident", "scan_host_list")}
    for _ in range(a.reps):
        events.start()
        trimmed, ms = wall(lambda: s.trim_reads(h, [ADAPTER], **call))
        t["trim_events"].append(events.stop_ms())
        t["trim_wall"].append(ms)
        (routed, _), ms = wall(host_route)
        t["host_route"].append(ms)
        routed.free()
        t["scan_resident"].append(wall(lambda: scan.hamming_best_pattern(pats, trimmed, 1))[1])
        t["scan_host_list"].append(wall(lambda: scan.hamming_best_pattern(pats, trimmed_list, 1))[1])
        trimmed.free()
    h.free()
    # the find kernel's walk: a read's rounds end with the one that accepts a position, else all of them
    lq, cut = rec["quality_len"].astype(np.int64), rec["adapter_pos"].astype(np.int64)
    count = np.where(lq >= a.min_overlap, lq - a.min_overlap + 1, 0)
    rounds = np.where(rec["adapter"] >= 0, cut // 64 + 1, (count + 63) // 64)
    valu = int(rounds.sum()) * (VALU_PER_ROUND + VALU_PER_ROUND_AND_ADAPTER)
    blocks = (layout - 64) // 64
    write_bytes = 2 * int(rec["length"].sum()) + 2 * layout + 4 * blocks + (16 + 48 + 16) * n  # what is read of text and quality, what is written
    b, c = statistics.median(t["trim_wall"]), statistics.median(t["host_route"])
    beyond = max(t["trim_wall"]) < min(t["host_route"]) or min(t["trim_wall"]) > max(t["host_route"])
    return {
        "input": {"reads": n, "read_len": READ_LEN, "fragments": "30..250 uniform", "substitutions": 0.01, "qualities": "33 + 38 falling by 26 over the read, +-10",
                  "adapter": ADAPTER.decode(), **call, "seed": a.seed},
        "result": {"with_adapter": int((rec["adapter"] >= 0).sum()), "dropped": int(((rec["length"] == 0)).sum()), "quality_cut": int((lq < READ_LEN).sum()),
                   "layout_bytes": layout, "trimmed_bases": int(rec["length"].sum())},
        "ms": {k: summary(v) for k, v in t.items()},
        "host_route_over_trim": round(c / b, 2), "ranges_apart": bool(beyond),
        "scan_host_list_over_resident": round(statistics.median(t["scan_host_list"]) / statistics.median(t["scan_resident"]), 2),
        "find_rounds": int(rounds.sum()), "find_valu": valu, "find_ms_at_issue_rate": round(valu * VALU_ISSUE_CYCLES / (SIMDS * CLOCK_HZ) * 1e3, 4),
        "write_bytes": write_bytes, "write_ms_at_peak": round(write_bytes / HBM_PEAK * 1e3, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--min-overlap", type=int, default=3)
    ap.add_argument("--max-permille", type=int, default=100)
    ap.add_argument("--quality-cutoff", type=int, default=20)
    ap.add_argument("--min-length", type=int, default=20)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--trace-run", action="store_true", help="warm-up and --reps trim calls per size, nothing written: the run a kernel trace wraps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trim_reads_bench.json"))
    a = ap.parse_args()
    import sassy_amd
    if sassy_amd.device_count() == 0:
        raise SystemExit("no HIP device visible: nothing is measured without one")
    if a.trace_run:
        for n in a.reads:
            run_size(sassy_amd, n, a, trace_only=True)
        return 0
    out = {"reps": a.reps, "version": sassy_amd.lib().sassy_hip_version().decode(), "sizes": [run_size(sassy_amd, n, a) for n in a.reads]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
