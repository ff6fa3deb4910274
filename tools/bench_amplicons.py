"""hamming_amplicons next to what a caller had to do before it, over the same device-resident text: device-generated DNA
with planted products, both alternated inside one repetition loop so that they see the same machine.  Run it in a fresh
process.

    python tools/bench_amplicons.py [--text-bytes 1000000000] [--reps 7] [--out profiles/amplicons_bench.json]

  amplicons   Searcher.hamming_amplicons(pairs, text, k, min_len, max_len)
  records     the yardstick: Searcher.search_hamming([F_0, R_0, F_1, R_1, ...], text, k, without_trace=True, as_result=True) on
              an rc searcher -- the same four scanned patterns per pair -- and a numpy join of its records on the host

16 pairs of 20-mers, k = 2, 100 <= L <= 2000; every pair has one planted product per 64 MiB of text, alternating between the
two orientations, each primer site with 0 .. 2 substitutions.  A second case, "short", is the one the call was made for: one
pair of 10-mers at k = 2 on the same text, where each scanned pattern has some 4 * 10^5 sites and the pair a few hundred
products.  Per run: wall_ms = the wall time of the whole step (for the
yardstick: the call and the join), call_ms = the library call's own wall time (stats total_ms), scan_ms = the HIP-event time
of the scan launches -- median, min, max and (max - min) / median over the repetitions.  The two arrays are compared for
equality in every repetition.
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

N_PAIRS, M, K, MIN_LEN, MAX_LEN = 16, 20, 2, 100, 2000
COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")
OTHER = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG"}


def revcomp(seq: bytes) -> bytes:
    return seq.translate(COMPLEMENT)[::-1]


def summary(v):
    med = statistics.median(v)
    return {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4), "spread": round((max(v) - min(v)) / med, 4) if med else 0.0}


def numpy_join(sassy_amd, arr, n_pairs, lens, min_len, max_len):
    """The amplicons from search_hamming's records of [F_0, R_0, F_1, R_1, ...] (rc searcher), in the contract's order."""
    import numpy as np
    out = []
    for i in range(n_pairs):
        a, b = lens[i]
        site = {}
        for p in (0, 1):
            for strand in (0, 1):
                sel = arr[(arr["pattern_idx"] == 2 * i + p) & (arr["strand"] == strand)]
                site[(p, strand)] = (sel["text_start"].astype(np.int64), sel["cost"].astype(np.int64))
        for strand in (0, 1):
            (ls, lc), (rs, rcost) = (site[(0, 0)], site[(1, 1)]) if strand == 0 else (site[(1, 0)], site[(0, 1)])
            width = b if strand == 0 else a
            shortest = max(min_len, a, b)
            if shortest > max_len or not len(ls) or not len(rs):
                continue
            first = np.searchsorted(rs, ls + shortest - width, side="left")
            last = np.searchsorted(rs, ls + max_len - width, side="right")
            cnt = np.maximum(last - first, 0)
            left = np.repeat(np.arange(len(ls)), cnt)
            right = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(first, cnt)
            rec = np.zeros(len(left), dtype=sassy_amd.amplicon_dtype())
            rec["start"], rec["end"], rec["pair_idx"], rec["strand"] = ls[left], rs[right] + width, i, strand
            rec["fwd_cost"] = lc[left] if strand == 0 else rcost[right]
            rec["rev_cost"] = rcost[right] if strand == 0 else lc[left]
            out.append(rec)
    return np.concatenate(out) if out else np.zeros(0, dtype=sassy_amd.amplicon_dtype())


def run_case(sassy_amd, np, buf, dev, n, rng, mutated, n_pairs, m, reps):
    pairs = [(bytes(rng.choice(b"ACGT") for _ in range(m)), bytes(rng.choice(b"ACGT") for _ in range(m))) for _ in range(n_pairs)]
    planted = 0
    for off in range(1 << 20, n - (n_pairs + 1) * 4096, 64 << 20):
        for i, (F, R) in enumerate(pairs):
            at, length = off + 4096 * i + 37 * i, rng.randrange(MIN_LEN, MAX_LEN + 1)
            left, right = (F, R) if (planted + i) % 2 == 0 else (R, F)
            buf.upload(mutated(left), at)
            buf.upload(mutated(revcomp(right)), at + length - m)
            planted += 1
    amp = sassy_amd.Searcher("dna", rc=True)
    rec = sassy_amd.Searcher("dna", rc=True)
    flat = [p for pair in pairs for p in pair]
    lens = [(len(f), len(r)) for f, r in pairs]

    def new_call():
        return amp.hamming_amplicons(pairs, dev, K, MIN_LEN, MAX_LEN)

    def yardstick():
        r = rec.search_hamming(flat, dev, K, without_trace=True, as_result=True)
        return numpy_join(sassy_amd, r.array, n_pairs, lens, MIN_LEN, MAX_LEN)

    runs = {"amplicons": (amp, new_call), "records": (rec, yardstick)}
    for _, fn in runs.values():  # warm-up: code objects, buffers
        for _ in range(2):
            fn()
    wall = {name: [] for name in runs}
    call = {name: [] for name in runs}
    scan = {name: [] for name in runs}
    info, agree = {}, True
    for _ in range(reps):  # alternated: every repetition runs both
        got = {}
        for name, (s, fn) in runs.items():
            t0 = time.perf_counter()
            got[name] = fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            st = s.stats()
            call[name].append(st["total_ms"])
            scan[name].append(st["scan_ms"])
            info[name] = {"scan_launches": int(st["scan_launches"]), "candidates": int(st["candidates"])}
        agree = agree and np.array_equal(got["amplicons"], got["records"])
    out = {"pairs": n_pairs, "m": m, "planted": planted, "records_found": int(len(got["amplicons"])), "arrays_agree": bool(agree), "runs": {}}
    for name in runs:
        out["runs"][name] = {"wall_ms": summary(wall[name]), "call_ms": summary(call[name]), "scan_ms": summary(scan[name]), **info[name],
                             "GB_per_s_wall": round(n / statistics.median(wall[name]) / 1e6, 1)}
    out["amplicons_over_records_wall"] = round(out["runs"]["amplicons"]["wall_ms"]["median"] / out["runs"]["records"]["wall_ms"]["median"], 4)
    return out, bool(agree) and len(got["amplicons"]) >= planted


def main():
    import numpy as np
    import sassy_amd
    from helpers.prose_text import DevText
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-bytes", type=float, default=1e9)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amplicons_bench.json"))
    a = ap.parse_args()
    n = int(a.text_bytes) // 64 * 64
    buf = sassy_amd.DeviceBuffer(n + 4096)
    sassy_amd.generate_dna(buf.ptr, n, 20261019)
    dev = DevText(buf.ptr, n)
    rng = random.Random(1)

    def mutated(seq):
        w = bytearray(seq)
        for j in rng.sample(range(len(w)), rng.randrange(K + 1)):
            w[j] = rng.choice(OTHER[w[j]])
        return bytes(w)

    out = {"text_bytes": n, "reps": a.reps, "k": K, "min_len": MIN_LEN, "max_len": MAX_LEN,
           "text": "generate_dna(seed 20261019), one product per pair per 64 MiB", "cases": {}}
    ok = True
    for case, n_pairs, m in (("primers", N_PAIRS, M), ("short", 1, 10)):
        res, good = run_case(sassy_amd, np, buf, dev, n, rng, mutated, n_pairs, m, a.reps)
        out["cases"][case] = res
        ok = ok and good
        print(json.dumps({case: res}), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    buf.free()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
