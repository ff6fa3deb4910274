"""Paired-end read overlap (Searcher.read_overlaps) over seeded synthetic pairs with both read batches resident on the device:
150-base reads cut from fragments of 50 .. 400 bases (a fragment shorter than the read is followed by random adapter bytes,
so read-through, ordinary overlap and no overlap all occur), 1 % substitutions in either read, Dna, min_overlap 10,
max_permille 200, k open.  Run it in a fresh process.

    python tools/bench_read_overlaps.py [--pairs 100000 1000000] [--reps 9] [--out profiles/read_overlaps_bench.json]
    python tools/bench_read_overlaps.py --trace-run          # the calls alone, for rocprofv3 --kernel-trace --stats

Per size, behind one warm-up call whose records are checked on a sample against tests/helpers/read_overlaps_ref.py:
  call_ms     the whole call between two device events (the Dna look at both batches, the kernel, the records' copy back
              and the host's waits), median, min, max and (max - min) / median of the repetitions
  kernel_ms   the library's own event pair around the kernel (stats: scan_ms), likewise -- the kernel trace of a separate
              run is the figure to quote for the kernel; this one is its cross-check
  pairs_per_s from the call's median
  bound       counted, not measured: the vector instructions of one offset round in the disassembly of the instantiation
              that runs (VALU_PER_ROUND; tools/overlap_loop_count.py counts them) times the rounds of every pair
              (overlap_step.h: ovl_offsets, 64 offsets a round), each instruction issued over VALU_ISSUE_CYCLES cycles per
              wavefront, over SIMDS x CLOCK_HZ.  The planes' construction and the reduction are outside of it
  hbm_bytes   what the call must move: both batches' sequence bytes once, 32 bytes of start and length tables and 16 bytes
              of record per pair
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

READ_LEN = 150
VALU_PER_ROUND = {6: 73}   # words per plane -> v_* instructions in the round loop of read_overlaps_kernel<6, false> (gfx950, -O3)
DS_PER_ROUND = {6: 18}     # ds_read_* of the same loop
VALU_ISSUE_CYCLES = 2      # a wavefront's vector instruction issues over 2 cycles (32 lanes a cycle)
SIMDS = 256 * 4
CLOCK_HZ = 2.4e9
HBM_PEAK = 8.0e12
COMP = np.zeros(256, dtype=np.uint8)
COMP[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)


def summary(v):
    med = statistics.median(v)
    return {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4), "spread": round((max(v) - min(v)) / med, 4) if med else 0.0}


def synthetic_pairs(n: int, seed: int):
    """(r1, r2, fragment lengths): two (n, 150) uint8 arrays of bases."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    frag_len = rng.integers(50, 401, n)
    frag = letters[rng.integers(0, 4, (n, 400), dtype=np.uint8)]
    cols = np.arange(READ_LEN)[None, :]
    adapter1 = letters[rng.integers(0, 4, (n, READ_LEN), dtype=np.uint8)]
    adapter2 = letters[rng.integers(0, 4, (n, READ_LEN), dtype=np.uint8)]
    rows = np.arange(n)[:, None]
    r1 = np.where(cols < frag_len[:, None], frag[rows, np.minimum(cols, 399)], adapter1)
    back = frag_len[:, None] - 1 - cols  # R2 reads the fragment's other strand from its far end
    r2 = np.where(back >= 0, COMP[frag[rows, np.maximum(back, 0)]], adapter2)
    for r in (r1, r2):  # 1 % substitutions (one that draws the same letter is none)
        hit = rng.random((n, READ_LEN)) < 0.01
        r[hit] = letters[rng.integers(0, 4, int(hit.sum()))]
    return np.ascontiguousarray(r1), np.ascontiguousarray(r2), frag_len


def fastq_bytes(reads: np.ndarray) -> np.ndarray:
    """minimal four-line FASTQ of an (n, L) array: '@', the bases, '+', an empty quality"""
    n, L = reads.shape
    grid = np.empty((n, L + 6), dtype=np.uint8)
    grid[:, :2] = np.frombuffer(b"@\n", dtype=np.uint8)
    grid[:, 2:2 + L] = reads
    grid[:, 2 + L:] = np.frombuffer(b"\n+\n\n", dtype=np.uint8)
    return grid.reshape(-1)


class Events:
    """Two HIP events on the default stream, through the runtime the library links."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def start(self):
        assert self.hip.hipEventRecord(self.a, None) == 0

    def stop_ms(self) -> float:
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return float(ms.value)


def rounds_of(la, lb, min_overlap):
    count = np.where((la >= min_overlap) & (lb >= min_overlap), la + lb - 2 * min_overlap + 1, 0)
    return (count + 63) // 64


def run_size(sassy_amd, n, a, trace_only=False):
    import read_overlaps_ref as oref
    r1, r2, frag_len = synthetic_pairs(n, a.seed)
    s = sassy_amd.Searcher("dna", rc=False)
    h1, h2 = sassy_amd.DeviceReads(fastq_bytes(r1)), sassy_amd.DeviceReads(fastq_bytes(r2))
    call = lambda: s.read_overlaps(h1, h2, a.min_overlap, 512, a.max_permille)  # noqa: E731
    got = call()  # warm-up, and the check on a sample
    sample = np.random.default_rng(1).choice(n, 300, replace=False)
    want = oref.expected_overlaps("dna", [r1[i].tobytes() for i in sample], [r2[i].tobytes() for i in sample], a.min_overlap, 512, a.max_permille)
    assert np.array_equal(got[sample], want), "the call and the definition disagree"
    if trace_only:
        for _ in range(a.reps):
            call()
        h1.free(); h2.free()
        return None
    events = Events()
    call_ms, kernel_ms = [], []
    for _ in range(a.reps):
        events.start()
        call()
        call_ms.append(events.stop_ms())
        kernel_ms.append(s.stats()["scan_ms"])
    words = int(s.stats()["word_rows"])
    seq_bytes = int(h1.seq_lens.sum() + h2.seq_lens.sum())
    h1.free(); h2.free()
    rounds = int(rounds_of(np.full(n, READ_LEN), np.full(n, READ_LEN), a.min_overlap).sum())
    valu = VALU_PER_ROUND.get(words)
    bound_ms = rounds * valu * VALU_ISSUE_CYCLES / (SIMDS * CLOCK_HZ) * 1e3 if valu else None
    hbm = seq_bytes + 32 * n + 16 * n
    k_med, c_med = statistics.median(kernel_ms), statistics.median(call_ms)
    found = got["n_accepted"] > 0
    return {
        "input": {"pairs": n, "read_len": READ_LEN, "fragments": "50..400 uniform", "substitutions": 0.01, "min_overlap": a.min_overlap,
                  "max_permille": a.max_permille, "k": 512, "seed": a.seed, "words_per_plane": words},
        "result": {"with_overlap": int(found.sum()), "read_through": int((found & (got["offset"] < 0)).sum()),
                   "several_accepted": int((got["n_accepted"] > 1).sum()),
                   "insert_equals_fragment": int((found & (np.where(got["offset"] >= 0, np.maximum(READ_LEN, got["offset"] + READ_LEN), got["overlap"]) == frag_len)).sum())},
        "call_ms": summary(call_ms), "kernel_ms_library_events": summary(kernel_ms),
        "pairs_per_s": round(n / (c_med / 1e3), 1), "pairs_per_s_kernel": round(n / (k_med / 1e3), 1),
        "bound": {"valu_per_round": valu, "ds_per_round": DS_PER_ROUND.get(words), "rounds": rounds, "issue_cycles": VALU_ISSUE_CYCLES, "simds": SIMDS,
                  "clock_hz": CLOCK_HZ, "bound_ms": round(bound_ms, 4) if bound_ms else None,
                  "kernel_over_bound": round(k_med / bound_ms, 2) if bound_ms else None},
        "hbm_bytes": hbm, "hbm_ms_at_peak": round(hbm / HBM_PEAK * 1e3, 4), "kernel_bytes_per_s": round(hbm / (k_med / 1e3), 1),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--min-overlap", type=int, default=10)
    ap.add_argument("--max-permille", type=int, default=200)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--trace-run", action="store_true", help="warm-up and --reps calls per size, nothing written: the run a kernel trace wraps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_overlaps_bench.json"))
    a = ap.parse_args()
    import sassy_amd
    if sassy_amd.device_count() == 0:
        raise SystemExit("no HIP device visible: nothing is measured without one")
    if a.trace_run:
        for n in a.pairs:
            run_size(sassy_amd, n, a, trace_only=True)
        return 0
    out = {"reps": a.reps, "version": sassy_amd.lib().sassy_hip_version().decode(), "sizes": [run_size(sassy_amd, n, a) for n in a.pairs]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
