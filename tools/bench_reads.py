"""search_many on a read set: P short patterns (barcodes) x many short texts (reads), both strands.

The shape of the reference's nanopore benchmark (96 x 24 bp vs 334 MB of reads, k = 3:
v2 116.8 GB/s pattern*text with 16 threads).  Synthetic reads: random ACGT, one planted barcode
(<= k edits) per read.

    python tools/bench_reads.py [--reads N] [--read-len L] [--patterns P] [--k K]

--min-costs / --best-pattern: the best-cost calls on the same reads and barcodes (same seed) next to search_many and to
search_many with without_trace + only_best_match (the nearest thing to them among the record calls): wall time of the
whole call from Python over a TextBatch, warmed, --reps repetitions, median and spread; one JSON line, also written to
--out (profiles/min_costs_bench.json).

--best-matches: Searcher.best_matches (default shape: 330 000 reads) next to the two ways to the same answer without it --
search_many followed by the host's reduction of its records, and search_many on an only_best_match searcher followed by
the same reduction -- and to best_pattern, the lower bound; --out defaults to profiles/best_matches_bench.json.

--device-parse: the same reads as FASTQ bytes in host memory, and per call (search_many as a numpy result, best_pattern,
best_matches), alternating inside one repetition loop after a warm-up that compares the results:
  (a) the call on the host texts (a TextBatch), against (b) the same call on the resident batch (sassy_amd.DeviceReads);
  (c) raw bytes -> results by the host reader (fastx's line table over the bytes) plus the call on its host texts, against
  (d) DeviceReads(raw) plus the call on it and the handle's release;
and the relayout alone: sassy_hip_reads_relayout of the whole batch into the separator layout between two device events (the
call uploads its start table and waits, so this bounds the kernel from above), bytes written per second.  Every timed leg ends
with a device synchronise.  One JSON line; --out defaults to profiles/reads_edit_resident.json.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import sassy_amd  # noqa: E402


def bench_best_cost(args, pats, texts, total):
    """Wall time of whole calls over one TextBatch: search_many (records as a numpy array), search_many without trace +
    only_best_match, and the best-cost calls asked for -- with the device reduction and with min_cost_device = 0."""
    batch = sassy_amd.TextBatch.from_list(texts)
    mk = lambda: sassy_amd.Searcher(args.profile, rc=not args.fwd, alpha=args.overhang)
    plain, best, new, host = mk(), mk().only_best_match(), mk(), mk()
    host.set_option("min_cost_device", 0)
    wo_flags = sassy_amd.WITHOUT_TRACE

    def search_many_wo(s):
        import ctypes as C
        pp, pl, n_p, tp, tl, n_t, _, _alive = s._marshal_many(pats, batch)
        out = C.c_void_p()
        sassy_amd._check(sassy_amd.lib().sassy_hip_search_many(s._h, pp, pl, n_p, tp, tl, n_t, args.k, wo_flags, C.byref(out)))
        return sassy_amd.Result(out)

    calls = {"search_many": lambda: plain.search_many(pats, batch, args.k, as_result=True),
             "search_many_without_trace_only_best": lambda: search_many_wo(best)}
    if args.min_costs:
        calls["min_costs"] = lambda: new.min_costs(pats, batch, args.k)
        calls["min_costs_general_path"] = lambda: host.min_costs(pats, batch, args.k)
    if args.best_pattern:
        calls["best_pattern"] = lambda: new.best_pattern(pats, batch, args.k)
        calls["best_pattern_general_path"] = lambda: host.best_pattern(pats, batch, args.k)
    if args.only_new:
        calls = {n: f for n, f in calls.items() if n in ("min_costs", "best_pattern")}
    res = {}
    for name, f in calls.items():
        f(); f()  # warm-up: kernels loaded, buffers grown
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = f()
            ts.append((time.perf_counter() - t0) * 1e3)
            del r
        ts = np.array(ts)
        res[name] = {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3),
                     "p10_ms": round(float(np.percentile(ts, 10)), 3), "p90_ms": round(float(np.percentile(ts, 90)), 3), "reps": args.reps}
    for name, s in (("min_costs" if args.min_costs else "best_pattern", new), ("search_many", plain)):
        if name not in calls:
            continue
        s.set_timing(2)
        calls[name]()
        st = s.stats()
        res[name]["kernel_ms_timing_level_2"] = {x: round(st[x], 3) for x in ("scan_ms", "filter_ms", "trace_ms")}
        res[name]["candidates"] = st["candidates"]
    doc = {"workload": f"{args.patterns} x {args.pattern_len} bp patterns, {args.reads} reads x {args.read_len} bp ({total / 1e6:.0f} MB), "
                       f"k={args.k}, {args.profile}, {'forward strand' if args.fwd else 'both strands'}",
           "what": "wall ms of the whole Python call over a TextBatch, warmed", "calls": res}
    line = json.dumps(doc)
    print(line)
    if args.out:
        prev = []
        if os.path.exists(args.out):
            with open(args.out) as fh:
                prev = json.load(fh)
        with open(args.out, "w") as fh:
            json.dump(prev + [doc], fh, indent=1)
            fh.write("\n")


def reduce_to_best(arr):
    """The best record per text of a search_many result by best_matches' definition, as row indices (numpy on the host:
    what a user does without the call)."""
    rc = arr["strand"].astype(bool)
    end = np.where(rc, arr["text_start"].astype(np.int64), -arr["text_end"].astype(np.int64))
    order = np.lexsort((end, arr["strand"], arr["pattern_idx"], arr["cost"], arr["text_idx"]))
    ti = arr["text_idx"][order]
    first = np.ones(len(order), dtype=bool)
    first[1:] = ti[1:] != ti[:-1]
    return order[first]


def bench_best_matches(args, pats, texts, total):
    batch = sassy_amd.TextBatch.from_list(texts)
    mk = lambda: sassy_amd.Searcher(args.profile, rc=not args.fwd, alpha=args.overhang)
    plain, only_best, new, host, lower = mk(), mk().only_best_match(), mk(), mk(), mk()
    host.set_option("best_match_device", 0)

    def via(s):
        r = s.search_many(pats, batch, args.k, as_result=True)
        return r, reduce_to_best(r.array)

    calls = {"search_many_then_host_reduction": lambda: via(plain),
             "search_many_only_best_match_then_host_reduction": lambda: via(only_best),
             "best_matches": lambda: new.best_matches(pats, batch, args.k, as_result=True),
             "best_matches_without_trace": lambda: new.best_matches(pats, batch, args.k, as_result=True, without_trace=True),
             "best_matches_general_path": lambda: host.best_matches(pats, batch, args.k, as_result=True),
             "best_pattern": lambda: lower.best_pattern(pats, batch, args.k)}
    if args.only_new:
        calls = {"best_matches": calls["best_matches"]}
    else:  # the same answer all ways
        r, idx = via(plain)
        want = r.array[idx]
        for name in ("best_matches", "best_matches_general_path"):
            got = calls[name]().array
            for f in ("text_idx", "pattern_idx", "cost", "strand", "text_start", "text_end", "pattern_start", "pattern_end", "cigar_len"):
                assert np.array_equal(got[f], want[f]), (name, f)
    res = {}
    for name, f in calls.items():
        f(); f()  # warm-up: kernels loaded, buffers grown
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = f()
            ts.append((time.perf_counter() - t0) * 1e3)
            del r
        ts = np.array(ts)
        res[name] = {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3),
                     "p10_ms": round(float(np.percentile(ts, 10)), 3), "p90_ms": round(float(np.percentile(ts, 90)), 3), "reps": args.reps}
    new.set_timing(2)
    n = len(calls["best_matches"]())
    st = new.stats()
    res["best_matches"]["records"] = n
    res["best_matches"]["candidates"] = st["candidates"]
    res["best_matches"]["kernel_ms_timing_level_2"] = {x: round(st[x], 3) for x in ("scan_ms", "filter_ms", "trace_ms")}
    doc = {"workload": f"{args.patterns} x {args.pattern_len} bp patterns, {args.reads} reads x {args.read_len} bp ({total / 1e6:.0f} MB), "
                       f"k={args.k}, {args.profile}, {'forward strand' if args.fwd else 'both strands'}",
           "what": "wall ms of the whole Python call over a TextBatch, warmed", "calls": res}
    print(json.dumps(doc))
    if args.out:
        prev = []
        if os.path.exists(args.out):
            with open(args.out) as fh:
                prev = json.load(fh)
        with open(args.out, "w") as fh:
            json.dump(prev + [doc], fh, indent=1)
            fh.write("\n")


def bench_device_parse(args, pats, texts, total):
    import ctypes as C
    from sassy_amd import fastx
    hip = C.CDLL("libamdhip64.so")
    n, L = len(texts), args.read_len
    head = 2 + 9 + 1
    row = head + L + 3 + L + 1
    grid = np.empty((n, row), dtype=np.uint8)
    grid[:, :2] = np.frombuffer(b"@r", dtype=np.uint8)
    digits = np.arange(n, dtype=np.int64)
    for d in range(9):
        grid[:, 2 + 8 - d] = ord("0") + digits % 10
        digits //= 10
    grid[:, head - 1] = 10
    grid[:, head:head + L] = np.frombuffer(b"".join(texts), dtype=np.uint8).reshape(n, L)
    grid[:, head + L:head + L + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    grid[:, head + L + 3:row - 1] = ord("I")
    grid[:, row - 1] = 10
    raw = grid.reshape(-1)
    mk = lambda: sassy_amd.Searcher(args.profile, rc=not args.fwd, alpha=args.overhang)
    s_host, s_dev = mk(), mk()
    sync = lambda: hip.hipDeviceSynchronize()
    calls = {"search_many": lambda s, t: s.search_many(pats, t, args.k, as_result=True).array,
             "best_pattern": lambda s, t: s.best_pattern(pats, t, args.k),
             "best_matches": lambda s, t: s.best_matches(pats, t, args.k, as_result=True).array}
    host_batch = fastx._parse_single_line_records(raw, 4).texts
    reads = sassy_amd.DeviceReads(raw)
    assert len(reads) == n and len(host_batch) == n

    def timed(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return (time.perf_counter() - t0) * 1e3, r

    def leg_c(call):
        return call(s_host, fastx._parse_single_line_records(raw, 4).texts)

    def leg_d(call):
        r = sassy_amd.DeviceReads(raw)
        out = call(s_dev, r)
        r.free()
        return out

    def same(x, y):
        if isinstance(x, tuple):
            return all(np.array_equal(a, b) for a, b in zip(x, y))
        return len(x) == len(y) and all(np.array_equal(x[f], y[f]) for f in ("pattern_idx", "text_idx", "text_start", "text_end", "cost", "strand", "cigar_len"))

    summary = lambda v: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3),
                         "spread": round(float((np.max(v) - np.min(v)) / np.median(v)), 4), "reps": len(v)}
    res = {}
    for name, call in calls.items():
        for _ in range(2):  # warm-up: kernels loaded, buffers grown; and the check
            a, b, c, d = call(s_host, host_batch), call(s_dev, reads), leg_c(call), leg_d(call)
        assert same(a, b) and same(a, c) and same(a, d), name
        st_host, st_dev = None, None
        ms = {"a_host_texts": [], "b_resident": [], "c_raw_host_reader": [], "d_raw_device_parse": []}
        for _ in range(args.reps):
            ms["a_host_texts"].append(timed(lambda: call(s_host, host_batch))[0])
            st_host = s_host.stats()
            ms["b_resident"].append(timed(lambda: call(s_dev, reads))[0])
            st_dev = s_dev.stats()
            ms["c_raw_host_reader"].append(timed(lambda: leg_c(call))[0])
            ms["d_raw_device_parse"].append(timed(lambda: leg_d(call))[0])
        res[name] = {k: summary(v) for k, v in ms.items()}
        res[name]["c_abi_total_ms_last_rep"] = {"a": round(st_host["total_ms"], 3), "b": round(st_dev["total_ms"], 3)}
        res[name]["path"] = {"filtered": [st_host["filtered"], st_dev["filtered"]], "scan_launches": [st_host["scan_launches"], st_dev["scan_launches"]]}
        print(name, json.dumps(res[name]), flush=True)
    # the relayout alone: the whole batch into the separator layout search_many_batched scans
    gap = (args.pattern_len + args.k + 1 + 15) // 16 * 16
    starts = np.arange(n, dtype=np.uint64) * np.uint64(L + gap)
    out_total = n * (L + gap) - gap
    buf = sassy_amd.DeviceBuffer(out_total + 64)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    rl = []
    for rep in range(args.reps + 2):
        assert hip.hipEventRecord(ev[0], None) == 0
        sassy_amd._check(sassy_amd.lib().sassy_hip_reads_relayout(reads._handle(), 0, n, starts.ctypes.data, out_total, ord("X"), buf.ptr, None))
        assert hip.hipEventRecord(ev[1], None) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]) == 0
        if rep >= 2:
            rl.append(float(t.value))
    buf.free()
    reads.free()
    med = float(np.median(rl))
    doc = {"workload": f"{args.patterns} x {args.pattern_len} bp patterns, {n} reads x {L} bp ({total / 1e6:.0f} MB of sequence, {raw.size / 1e6:.0f} MB of FASTQ), "
                       f"k={args.k}, {args.profile}, {'forward strand' if args.fwd else 'both strands'}",
           "what": "wall ms of whole Python calls, a device synchronise at the end of each, legs alternating in one loop, warmed",
           "calls": res,
           "relayout_call": dict(summary(rl), bytes_written=int(out_total), bytes_read=int(total),
                                 written_gb_per_s=round(out_total / 1e9 / (med / 1e3), 1), moved_gb_per_s=round((out_total + total) / 1e9 / (med / 1e3), 1),
                                 what="device events around sassy_hip_reads_relayout (start table upload, kernel, wait)")}
    print(json.dumps(doc))
    if args.out:
        prev = []
        if os.path.exists(args.out):
            with open(args.out) as fh:
                prev = json.load(fh)
        with open(args.out, "w") as fh:
            json.dump(prev + [doc], fh, indent=1)
            fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=None, help="default 100 000; 330 000 with --best-matches")
    ap.add_argument("--read-len", type=int, default=1000)
    ap.add_argument("--patterns", type=int, default=96)
    ap.add_argument("--pattern-len", type=int, default=24)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--profile", default="iupac")
    ap.add_argument("--overhang", type=float, default=None)
    ap.add_argument("--fwd", action="store_true", help="forward strand only (the reference's nanopore bench, evals/src/sassy2/bench.rs)")
    ap.add_argument("--min-costs", action="store_true", help="time Searcher.min_costs next to search_many")
    ap.add_argument("--best-pattern", action="store_true", help="time Searcher.best_pattern next to search_many")
    ap.add_argument("--best-matches", action="store_true", help="time Searcher.best_matches next to search_many + host reduction")
    ap.add_argument("--device-parse", action="store_true", help="the calls on host texts against the same calls on a resident read batch (DeviceReads)")
    ap.add_argument("--only-new", action="store_true", help="with --min-costs / --best-pattern / --best-matches: only these calls' device path (a kernel trace of it alone)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="default profiles/min_costs_bench.json; profiles/best_matches_bench.json with --best-matches")
    args = ap.parse_args()
    if args.reads is None:
        args.reads = 330_000 if args.best_matches else 100_000
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "reads_edit_resident.json" if args.device_parse else
                                "best_matches_bench.json" if args.best_matches else "min_costs_bench.json")
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    pats = [bytes(acgt[rng.integers(0, 4, args.pattern_len)]) for _ in range(args.patterns)]
    flat = acgt[rng.integers(0, 4, args.reads * args.read_len)].reshape(args.reads, args.read_len).copy()
    which = rng.integers(0, args.patterns, args.reads)
    at = rng.integers(0, args.read_len - args.pattern_len, args.reads)
    for r in range(args.reads):
        p = np.frombuffer(pats[which[r]], dtype=np.uint8)
        flat[r, at[r]:at[r] + args.pattern_len] = p
    texts = [flat[r].tobytes() for r in range(args.reads)]
    total = args.reads * args.read_len
    if args.device_parse:
        return bench_device_parse(args, pats, texts, total)
    if args.best_matches:
        return bench_best_matches(args, pats, texts, total)
    if args.min_costs or args.best_pattern:
        return bench_best_cost(args, pats, texts, total)
    s = sassy_amd.Searcher(args.profile, rc=not args.fwd, alpha=args.overhang)
    s.search_many(pats[:2], texts[:100], args.k)  # warm-up (kernels loaded)
    s.search_many(pats, texts, args.k)             # first full-size call: grows the staging / device buffers
    first_ms = s.stats()["total_ms"]
    dts, sts = [], []
    for _ in range(3):                              # steady state: the best of three calls (each one's C-ABI time is listed)
        t0 = time.perf_counter()
        ms = s.search_many(pats, texts, args.k, as_result=True)  # (the records as a numpy array: no Python object per match)
        dts.append(time.perf_counter() - t0)
        sts.append(s.stats())
    best = min(range(3), key=lambda i: sts[i]["total_ms"])
    dt, st = dts[best], sts[best]
    batch = sassy_amd.TextBatch.from_list(texts)  # the same read set as one buffer + offsets: nothing per text in Python
    t0 = time.perf_counter()
    ms_b = s.search_many(pats, batch, args.k, as_result=True)
    dt_batch = time.perf_counter() - t0
    assert len(ms_b) == len(ms)
    print(json.dumps({
        "workload": f"{args.patterns} x {args.pattern_len} bp patterns, {args.reads} reads x {args.read_len} bp "
                    f"({total / 1e6:.0f} MB), k={args.k}, {args.profile}, {'forward strand' if args.fwd else 'both strands'}"
                    + (f", overhang {args.overhang}" if args.overhang is not None else ""),
        "seconds_python_call": round(dt, 3), "seconds_python_call_text_batch": round(dt_batch, 3), "seconds_c_abi": round(st["total_ms"] / 1e3, 4), "seconds_c_abi_each_call": [round(x["total_ms"] / 1e3, 4) for x in sts],
        "seconds_c_abi_first_call": round(first_ms / 1e3, 3),
        "pattern_text_GB_per_s": round(total * args.patterns / (st["total_ms"] / 1e3) / 1e9, 1),
        "matches": len(ms), "scan_launches": st["scan_launches"], "scan_kernel_ms": round(st["scan_ms"], 2),
        "host_ms": {k: round(st[k], 1) for k in ("host_enqueue_ms", "host_wait_ms", "host_post_ms")},
    }))


if __name__ == "__main__":
    main()
