"""All-vs-all Hamming distances (Searcher.hamming_pairs / hamming_nearest) on whitelist- and barcode-shaped inputs.

    python tools/bench_hamming_pairs.py [--reads 1000000] [--reps 5] [--out profiles/hamming_pairs.txt]

  (1) against the sliding path's way to the same answer: hamming_nearest(reads, whitelist, 1) and
      hamming_best_pattern(whitelist, reads, 1) on random 16-mer reads -- half of them whitelist entries with 0 .. 2
      substitutions --, whitelists of 1 000 / 10 000 / 100 000 entries, Dna, rc off and on; the two legs alternate inside one
      repetition loop and their (cost, index, strand) are compared.  The sliding leg of a size is run once, and left out
      when the smaller sizes' times, scaled by the whitelist, say it would take longer than --old-budget-s.
  (2) shapes the sliding path cannot take: self-mode hamming_pairs on 100 000 and 1 000 000 16-mers at k = 1 and 2, and
      hamming_nearest of the reads against a whitelist of 4 000 000 entries, with the time per pass (timing level 2: survey,
      scan or reduce, fill).
  (3) the inner loop: pairs per second of the survey pass alone against the vector issue rate, for the instruction count per
      pair and strand read off the compiler's ISA (--valu-per-pair, DESIGN.md 5.10 "Pairs").

Times are wall-clock milliseconds of the whole call (median, min and max over the repetitions); "pairs" are (entry, target,
strand) comparisons the call is defined over, per second of wall time.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
CUS, SIMDS, CLOCK_HZ = 256, 4, 2.4e9


def random_rows(rng, n, m):
    return LETTERS[rng.integers(0, 4, size=(n, m))]


def reads_from(rng, whitelist, n, m):
    """n reads: even ones a whitelist entry with 0 .. 2 substitutions, odd ones random"""
    reads = random_rows(rng, n, m)
    src = rng.integers(0, len(whitelist), size=n // 2)
    reads[0::2][:len(src)] = whitelist[src]
    for d in (1, 2):
        rows = np.arange(0, 2 * len(src), 2)[rng.integers(0, 3, size=len(src)) >= d]
        cols = rng.integers(0, m, size=len(rows))
        reads[rows, cols] = LETTERS[rng.integers(0, 4, size=len(rows))]
    return reads


def timed(fn, reps):
    fn()  # warm-up: code objects, buffers
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def line(out, text):
    print(text, flush=True)
    out.append(text)


def spread(ms):
    return f"{statistics.median(ms):10.2f} ms (min {min(ms):.2f}, max {max(ms):.2f})"


def main():
    import sassy_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("-m", type=int, default=16)
    ap.add_argument("--whitelists", default="1000,10000,100000")
    ap.add_argument("--self-sizes", default="100000,1000000")
    ap.add_argument("--big-whitelist", type=int, default=4000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-budget-s", type=float, default=60.0)
    ap.add_argument("--valu-per-pair", type=float, default=4.75, help="vector instructions per pair and strand in the Dna W = 1 loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hamming_pairs.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261019)
    out = []
    line(out, f"# tools/bench_hamming_pairs.py: {a.reads} reads of {a.m} bases, Dna, reps {a.reps}; {sassy_amd.lib().sassy_hip_version().decode()}")

    # ---- (1) against the sliding path
    line(out, "# (1) hamming_nearest(reads, whitelist, 1) vs hamming_best_pattern(whitelist, reads, 1)")
    old_s_per_entry = None
    for rc in (False, True):
        for n_w in [int(x) for x in a.whitelists.split(",")]:
            whitelist = random_rows(rng, n_w, a.m)
            reads = reads_from(rng, whitelist, a.reads, a.m)
            s = sassy_amd.Searcher("dna", rc=rc)
            new = {}
            ms_new = timed(lambda: new.update(r=s.hamming_nearest(reads, whitelist, 1)), a.reps)
            pairs = a.reads * n_w * (2 if rc else 1)
            med = statistics.median(ms_new)
            line(out, f"rc={int(rc)} whitelist={n_w:7d} nearest      {spread(ms_new)}  {pairs / med / 1e6:10.1f} G pairs/s  found={(new['r'][0] != sassy_amd.NO_MATCH).sum()}")
            estimate = None if old_s_per_entry is None else old_s_per_entry * n_w * (2 if rc else 1)
            if estimate is not None and estimate > a.old_budget_s:
                line(out, f"rc={int(rc)} whitelist={n_w:7d} best_pattern  left out: about {estimate:.0f} s by the smaller sizes' time per whitelist entry and strand")
                continue
            batch = sassy_amd.TextBatch.from_list([r.tobytes() for r in reads])
            pats = [r.tobytes() for r in whitelist]
            old = {}
            t0 = time.perf_counter()
            old.update(r=s.hamming_best_pattern(pats, batch, 1))
            first = time.perf_counter() - t0
            ms_old = [first * 1e3] if first > 5 else timed(lambda: old.update(r=s.hamming_best_pattern(pats, batch, 1)), max(1, a.reps // 2))
            med_old = statistics.median(ms_old)
            old_s_per_entry = max(old_s_per_entry or 0.0, med_old / 1e3 / (n_w * (2 if rc else 1)))
            same = all((x == y).all() for x, y in zip(new["r"][:3], old["r"][:3]))
            line(out, f"rc={int(rc)} whitelist={n_w:7d} best_pattern {spread(ms_old)}  {pairs / med_old / 1e6:10.1f} G pairs/s  same answer={same}  ratio old/new={med_old / med:.1f}")

    # ---- (2) shapes the sliding path cannot take
    line(out, "# (2) self-mode hamming_pairs; hamming_nearest against a large whitelist; per pass at timing level 2")
    s = sassy_amd.Searcher("dna", rc=False)
    s.set_timing(2)
    survey_rate = {}
    for n in [int(x) for x in a.self_sizes.split(",")]:
        seqs = random_rows(rng, n, a.m)
        for k in (1, 2):
            got = {}
            ms = timed(lambda: got.update(r=s.hamming_pairs(seqs, None, k)), a.reps)
            st = s.stats()
            pairs = n * (n - 1) // 2
            med = statistics.median(ms)
            line(out, f"self n={n:8d} k={k} pairs        {spread(ms)}  {pairs / med / 1e6:10.1f} G pairs/s  records={len(got['r'])}  "
                      f"survey {st['filter_ms']:.2f} ms  scan {st['scan_ms'] - st['filter_ms'] - st['trace_ms']:.3f} ms  fill {st['trace_ms']:.2f} ms  "
                      f"chunks={st['chunks']}")
            survey_rate[f"self n={n} k={k}"] = pairs / (st["filter_ms"] / 1e3)
    whitelist = random_rows(rng, a.big_whitelist, a.m)
    reads = reads_from(rng, whitelist, a.reads, a.m)
    got = {}
    ms = timed(lambda: got.update(r=s.hamming_nearest(reads, whitelist, 1)), max(1, a.reps // 2))
    st = s.stats()
    pairs = a.reads * a.big_whitelist
    med = statistics.median(ms)
    line(out, f"nearest reads={a.reads} whitelist={a.big_whitelist} {spread(ms)}  {pairs / med / 1e6:10.1f} G pairs/s  "
              f"found={(got['r'][0] != sassy_amd.NO_MATCH).sum()} unambiguous={(got['r'][3] == 1).sum()}  "
              f"survey {st['filter_ms']:.2f} ms  reduce {st['scan_ms'] - st['filter_ms']:.3f} ms  chunks={st['chunks']}")
    survey_rate["nearest, large whitelist"] = pairs / (st["filter_ms"] / 1e3)

    # ---- (3) the inner loop against the vector issue rate
    line(out, f"# (3) survey pass alone, {a.valu_per_pair} vector instructions per pair and strand (Dna, W = 1); issue rate = "
              f"{CUS} CUs x {SIMDS} SIMDs x lanes per clock x {CLOCK_HZ / 1e9:.1f} GHz")
    for name, rate in survey_rate.items():
        lane_ops = rate * a.valu_per_pair
        line(out, f"{name:32s} {rate / 1e12:7.3f} T pairs/s  = {lane_ops / (CUS * SIMDS * 32 * CLOCK_HZ):.3f} of the rate at 32 lanes per clock and SIMD, "
                  f"{lane_ops / (CUS * SIMDS * 16 * CLOCK_HZ):.3f} at 16")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
