"""UMI grouping (Searcher.umi_groups) next to the call it grew out of: Searcher.hamming_clusters on the same list, which walks
every read against every other read where umi_groups collapses the duplicates first and walks the distinct sequences only.

    python tools/bench_umi_groups.py [--reps 5] [--out profiles/umi_groups.txt]

The shapes are those of tools/bench_clusters.py (Dna 16-mers, k = 1):
  (1) sparse: 10^5 and 10^6 random sequences -- next to no duplicates, so the collapse is pure overhead: its share of the call
      is stated.
  (2) dense: 10^6 reads drawn from 10^4, 10^3 and 10^2 UMIs, every second read with one substitution -- n_u << n, the walk is
      over n_u^2 / 2 pairs.

Per shape: the baseline, method="cluster" (which must return the baseline's labels and sizes, or the tool stops) and
method="directional"; wall-clock milliseconds of the whole call (median, min and max over the repetitions, behind one warm-up
call) and HIP-event milliseconds per pass at timing level 2 -- the collapse (table, lookup, scan, gather), the walk passes over
the distinct sequences, the relaxation with the size and expand passes --, n_u, the records among the distinct sequences and
the relaxation's launches.  method="unique" is the collapse alone.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_clusters import line, random_rows, spread, timed, umi_reads  # noqa: E402


def main():
    import sassy_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("-m", type=int, default=16)
    ap.add_argument("--sparse", default="100000,1000000")
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--umis", default="10000,1000,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umi_groups.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261020)
    out = []
    line(out, f"# tools/bench_umi_groups.py: Dna, {a.m} bases, k = 1, reps {a.reps}; {sassy_amd.lib().sassy_hip_version().decode()}")
    s = sassy_amd.Searcher("dna", rc=False)
    s.set_timing(2)

    def shape(tag, seqs):
        n = len(seqs)
        got = {}
        ms = timed(lambda: got.update(r=s.hamming_clusters(seqs, 1)), a.reps)
        st = s.stats()
        base, base_labels, base_sizes = statistics.median(ms), *got["r"]
        line(out, f"{tag} hamming_clusters      {spread(ms)}  clusters={int((base_labels == np.arange(n)).sum())}  link {st['filter_ms']:.2f} ms  chunks={st['chunks']}")
        medians = {}
        for method in ("unique", "cluster", "directional"):
            ms = timed(lambda: got.update(r=s.umi_groups(seqs, 1, method)), a.reps)
            st = s.stats()
            labels, sizes, reps, _ = got["r"]
            if method == "cluster" and not (np.array_equal(labels, base_labels) and np.array_equal(sizes, base_sizes)):
                raise SystemExit(f"{tag}: method=cluster and hamming_clusters disagree")
            med = medians[method] = statistics.median(ms)
            collapse = st["scan_ms"] - st["filter_ms"] - st["trace_ms"]
            line(out, f"{tag} umi {method:12s}      {spread(ms)}  groups={int((labels == np.arange(n)).sum())} n_u={st['hit_blocks']} records={st['candidates']} "
                      f"rounds={st['blocks']}  collapse {collapse:.2f} ms ({100 * collapse / med:.0f} % of the call)  walk {st['filter_ms']:.2f} ms  "
                      f"relax+expand {st['trace_ms']:.2f} ms  chunks={st['chunks']}")
        line(out, f"{tag} cluster / baseline = {medians['cluster'] / base:.2f} of the time; directional / baseline = {medians['directional'] / base:.2f}")

    line(out, "# (1) sparse: random sequences, next to no duplicates -- the collapse is overhead")
    for n in [int(x) for x in a.sparse.split(",")]:
        shape(f"sparse n={n:8d}", random_rows(rng, n, a.m))
    line(out, f"# (2) dense: {a.reads} reads from U UMIs, 0 or 1 substitutions each")
    for umis in [int(x) for x in a.umis.split(",")]:
        shape(f"dense U={umis:6d}", umi_reads(rng, a.reads, umis, a.m))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
