"""Sequence clustering (Searcher.hamming_clusters / edit_clusters) next to the way to the same answer without it: the
self-mode pair records (Searcher.hamming_pairs / edit_pairs) and a union of them on the host.

    python tools/bench_clusters.py [--reps 5] [--out profiles/clusters.txt]

  (1) sparse: 10^5 and 10^6 random Dna 16-mers at k = 1 and 2 (the edit calls at 10^5 only) -- a handful of records, the walk
      is all there is.  The link pass beside the survey pass of the pair call on the same list.
  (2) dense: 10^6 reads drawn from 10^4, 10^3 and 10^2 UMIs, each read its UMI with 0 or 1 substitutions, at k = 1 -- the
      records grow with the square of the copies per UMI.  The record path is run while the pairs inside the clusters (an
      upper bound of its records, read off the clustering's own sizes) stay below --baseline-records; beyond that its
      records and bytes are stated, not made.

Times are wall-clock milliseconds of the whole call (median, min and max over the repetitions; the dense record path runs
once behind its warm-up) and HIP-event milliseconds per pass (timing level 2).  Both ways must give the same labels, or the tool stops.
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


def random_rows(rng, n, m):
    return LETTERS[rng.integers(0, 4, size=(n, m))]


def umi_reads(rng, n, umis, m):
    """n reads: a random one of `umis` random sequences, every second read with one base changed to another letter"""
    centres = random_rows(rng, umis, m)
    reads = centres[rng.integers(0, umis, size=n)]
    rows = np.flatnonzero(rng.integers(0, 2, size=n))
    cols = rng.integers(0, m, size=len(rows))
    code = (reads[rows, cols] >> 1) & 3
    reads[rows, cols] = np.frombuffer(b"ACTG", dtype=np.uint8)[(code + rng.integers(1, 4, size=len(rows))) % 4]  # (code: A C T G)
    return np.ascontiguousarray(reads)


def union_on_host(n, records):
    """the labels (smallest index per component) of the records' graph: every node takes the smallest label across its
    edges, then its label's label, until nothing moves (the edges grouped by either end once, a segmented minimum per turn)"""
    i, j = records["a_idx"].astype(np.int64), records["b_idx"].astype(np.int64)
    lab = np.arange(n, dtype=np.int64)
    if not len(i):
        return lab.astype(np.uint32)
    ends = []
    for end in (i, j):
        order = np.argsort(end, kind="stable")
        ordered = end[order]
        starts = np.flatnonzero(np.r_[True, ordered[1:] != ordered[:-1]])
        ends.append((order, starts, ordered[starts]))
    while True:
        low = np.minimum(lab[i], lab[j])
        new = lab.copy()
        for order, starts, nodes in ends:
            new[nodes] = np.minimum(new[nodes], np.minimum.reduceat(low[order], starts))
        new = new[new]
        if np.array_equal(new, lab):
            return lab.astype(np.uint32)
        lab = new


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
    ap.add_argument("-m", type=int, default=16)
    ap.add_argument("--sparse", default="100000,1000000")
    ap.add_argument("--edit-limit", type=int, default=100000, help="the edit calls run on lists of at most this many sequences")
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--umis", default="10000,1000,100")
    ap.add_argument("--baseline-records", type=float, default=1e8, help="run the record path while the clusters hold at most this many pairs")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clusters.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261020)
    out = []
    line(out, f"# tools/bench_clusters.py: Dna, {a.m} bases, reps {a.reps}; {sassy_amd.lib().sassy_hip_version().decode()}")
    s = sassy_amd.Searcher("dna", rc=False)
    s.set_timing(2)

    def clustering(tag, name, seqs, k):
        call = s.edit_clusters if name == "edit" else s.hamming_clusters
        got = {}
        ms = timed(lambda: got.update(r=call(seqs, k)), a.reps)
        st = s.stats()
        labels, sizes = got["r"]
        roots = labels == np.arange(len(seqs))
        inside = int((sizes[roots].astype(np.int64) * (sizes[roots].astype(np.int64) - 1) // 2).sum())
        line(out, f"{tag} {name + '_clusters':17s} {spread(ms)}  clusters={int(roots.sum())} largest={int(sizes.max())} pairs inside={inside}  "
                  f"link {st['filter_ms']:.2f} ms  flatten {st['scan_ms'] - st['filter_ms']:.3f} ms  chunks={st['chunks']}")
        return labels, inside, statistics.median(ms), st["filter_ms"]

    def record_path(tag, name, seqs, k, labels, cluster_ms, link_ms, reps):
        call = s.edit_pairs if name == "edit" else s.hamming_pairs
        got = {}

        def both():
            t0 = time.perf_counter()
            records = call(seqs, None, k)
            got["pairs_ms"] = (time.perf_counter() - t0) * 1e3
            got["records"] = len(records)
            got["labels"] = union_on_host(len(seqs), records)
        ms = timed(both, reps)
        st = s.stats()
        if not np.array_equal(got["labels"], labels):
            raise SystemExit(f"{tag}: the two ways disagree")
        med = statistics.median(ms)
        line(out, f"{tag} {name + '_pairs + union':17s} {spread(ms)}  records={got['records']} ({got['records'] * 12 / 1e6:.1f} MB)  pairs call {got['pairs_ms']:.2f} ms  "
                  f"survey {st['filter_ms']:.2f} ms  fill {st['trace_ms']:.2f} ms  chunks={st['chunks']}")
        line(out, f"{tag} {name}: clusters / records path = {cluster_ms / med:.2f} of the time; link / survey = {link_ms / st['filter_ms']:.2f}")

    line(out, "# (1) sparse: random sequences; the clustering call, below it the self-mode pair call and a union on the host")
    for n in [int(x) for x in a.sparse.split(",")]:
        seqs = random_rows(rng, n, a.m)
        for name in ("hamming", "edit"):
            if name == "edit" and n > a.edit_limit:
                continue
            for k in (1, 2):
                tag = f"sparse n={n:8d} k={k}"
                labels, _, ms, link = clustering(tag, name, seqs, k)
                record_path(tag, name, seqs, k, labels, ms, link, a.reps)

    line(out, f"# (2) dense: {a.reads} reads from U UMIs, 0 or 1 substitutions each, k = 1")
    for umis in [int(x) for x in a.umis.split(",")]:
        seqs = umi_reads(rng, a.reads, umis, a.m)
        tag = f"dense U={umis:6d}"
        labels, inside, ms, link = clustering(tag, "hamming", seqs, 1)
        if inside <= a.baseline_records:
            record_path(tag, "hamming", seqs, 1, labels, ms, link, 1)  # (once: hundreds of megabytes of records)
        else:
            limit = "hamming_pairs refuses more than 2^32 - 1 records" if inside > 0xFFFFFFFF else "below the call's limit of 2^32 - 1 records"
            line(out, f"{tag} record path not run: up to {inside} records = {inside * 12 / 1e9:.1f} GB on the device and again on the host ({limit})")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
