"""All-vs-all edit distances (Searcher.edit_pairs / edit_nearest) on whitelist- and barcode-shaped inputs, each shape next to
the Hamming call on the same lists as its floor (the same walk with a popcount where the column steps are).

    python tools/bench_edit_pairs.py [--reads 1000000] [--reps 5] [--out profiles/edit_pairs.txt]

  (1) edit_nearest(reads, whitelist, 1) on random 16-mer reads -- half of them whitelist entries with 0 .. 2 edits, a third
      of the edits a lost or a gained base --, whitelists of 10 000 and 100 000 entries, Dna.
  (2) self-mode edit_pairs on 100 000 16-mers at k = 1 and 2.
  (3) one two-word shape: edit_nearest of 100 000 64-mers against 10 000, k = 3.
  (4) the inner loop: pairs per second of the survey pass alone against the vector issue rate, for the instruction count per
      pair read off the compiler's ISA (--valu-per-pair, DESIGN.md 5.10 "Edit pairs").

Times are wall-clock milliseconds of the whole call (median, min and max over the repetitions) and HIP-event milliseconds per
pass (timing level 2: survey, scan or reduce, fill); "pairs" are the (entry, target) comparisons the call is defined over.
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
    """n reads: even ones a whitelist entry with 0 .. 2 edits (substitution, lost base, gained base), odd ones random"""
    reads = random_rows(rng, n, m)
    half = n // 2
    rows = whitelist[rng.integers(0, len(whitelist), size=half)]
    cols = np.arange(m)[None, :]
    for d in (1, 2):
        hit = rng.integers(0, 3, size=half) >= d
        op = rng.integers(0, 3, size=half)
        pos = rng.integers(0, m, size=half)[:, None]
        fresh = LETTERS[rng.integers(0, 4, size=half)][:, None]
        wide = np.concatenate([rows, fresh], axis=1)
        lost = np.take_along_axis(wide, cols + (cols >= pos), axis=1)                       # row[pos] dropped, a new last base
        gained = np.where(cols == pos, fresh, np.take_along_axis(rows, cols - (cols > pos), axis=1))  # a base put in at pos
        changed = np.where(cols == pos, fresh, rows)
        edited = np.where((op == 0)[:, None], changed, np.where((op == 1)[:, None], lost, gained))
        rows = np.where(hit[:, None], edited, rows)
    reads[0::2][:half] = rows
    return np.ascontiguousarray(reads)


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


def passes(st, last):
    return (f"survey {st['filter_ms']:.2f} ms  {'scan' if last else 'reduce'} {st['scan_ms'] - st['filter_ms'] - st['trace_ms']:.3f} ms"
            + (f"  fill {st['trace_ms']:.2f} ms" if last else "") + f"  chunks={st['chunks']}")


def main():
    import sassy_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("-m", type=int, default=16)
    ap.add_argument("--whitelists", default="10000,100000")
    ap.add_argument("--self-size", type=int, default=100000)
    ap.add_argument("--long-m", type=int, default=64)
    ap.add_argument("--long-reads", type=int, default=100000)
    ap.add_argument("--long-whitelist", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--valu-per-pair", type=float, default=250.0, help="vector instructions per pair in the Dna W = 1 survey loop at m_b = 16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_pairs.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261020)
    out = []
    line(out, f"# tools/bench_edit_pairs.py: {a.reads} reads of {a.m} bases, Dna, reps {a.reps}; {sassy_amd.lib().sassy_hip_version().decode()}")
    s = sassy_amd.Searcher("dna", rc=False)
    s.set_timing(2)
    survey_rate = {}

    def nearest_pair(tag, reads, whitelist, k):
        got = {}
        pairs = len(reads) * len(whitelist)
        for name, call in (("edit_nearest", s.edit_nearest), ("hamming_nearest", s.hamming_nearest)):
            ms = timed(lambda: got.update({name: call(reads, whitelist, k)}), a.reps)
            st = s.stats()
            med = statistics.median(ms)
            r = got[name]
            line(out, f"{tag} {name:16s} {spread(ms)}  {pairs / med / 1e6:9.1f} G pairs/s  found={(r[0] != sassy_amd.NO_MATCH).sum()} "
                      f"unambiguous={(r[3] == 1).sum()}  {passes(st, False)}")
            if name == "edit_nearest":
                survey_rate[tag] = pairs / (st["filter_ms"] / 1e3)
        e, h = got["edit_nearest"], got["hamming_nearest"]
        line(out, f"{tag} entries found under E only: {((e[0] != sassy_amd.NO_MATCH) & (h[0] == sassy_amd.NO_MATCH)).sum()}; "
                  f"E <= H everywhere: {bool((e[0] <= h[0]).all())}")

    line(out, "# (1) edit_nearest(reads, whitelist, 1), below it hamming_nearest on the same lists")
    for n_w in [int(x) for x in a.whitelists.split(",")]:
        whitelist = random_rows(rng, n_w, a.m)
        nearest_pair(f"m={a.m} reads={a.reads} whitelist={n_w:7d}", reads_from(rng, whitelist, a.reads, a.m), whitelist, 1)

    line(out, "# (2) self-mode edit_pairs, below it hamming_pairs on the same list")
    seqs = random_rows(rng, a.self_size, a.m)
    for k in (1, 2):
        for name, call in (("edit_pairs", s.edit_pairs), ("hamming_pairs", s.hamming_pairs)):
            got = {}
            ms = timed(lambda: got.update(r=call(seqs, None, k)), a.reps)
            st = s.stats()
            pairs = a.self_size * (a.self_size - 1) // 2
            med = statistics.median(ms)
            line(out, f"self n={a.self_size} k={k} {name:14s} {spread(ms)}  {pairs / med / 1e6:9.1f} G pairs/s  records={len(got['r'])}  {passes(st, True)}")
            if name == "edit_pairs":
                survey_rate[f"self n={a.self_size} k={k}"] = pairs / (st["filter_ms"] / 1e3)

    line(out, f"# (3) two words per plane: m = {a.long_m}, k = 3")
    whitelist = random_rows(rng, a.long_whitelist, a.long_m)
    tag = f"m={a.long_m} reads={a.long_reads} whitelist={a.long_whitelist:7d}"
    nearest_pair(tag, reads_from(rng, whitelist, a.long_reads, a.long_m), whitelist, 3)
    long_rate = survey_rate.pop(tag)
    line(out, f"{tag} survey alone: {long_rate / 1e9:.1f} G pairs/s = {long_rate * a.long_m / 1e12:.3f} T columns/s")

    line(out, f"# (4) survey pass alone, {a.valu_per_pair} vector instructions per pair (Dna, W = 1, {a.m} columns); issue rate = "
              f"{CUS} CUs x {SIMDS} SIMDs x lanes per clock x {CLOCK_HZ / 1e9:.1f} GHz")
    for name, rate in survey_rate.items():
        lane_ops = rate * a.valu_per_pair
        line(out, f"{name:44s} {rate / 1e9:8.1f} G pairs/s  = {lane_ops / (CUS * SIMDS * 32 * CLOCK_HZ):.3f} of the rate at 32 lanes per clock and SIMD, "
                  f"{lane_ops / (CUS * SIMDS * 16 * CLOCK_HZ):.3f} at 16")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
