"""Counts the instructions of the offset-round loop of every read_overlaps_kernel instantiation in the device assembly (the
figures tools/bench_read_overlaps.py derives its bound from):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S sassy_amd/csrc/read_overlaps.hip -o ro.s
    python tools/overlap_loop_count.py ro.s

Per kernel the outermost block that ends in a backward branch -- the round loop -- is taken: its instructions, how many are
vector ALU (v_*), LDS (ds_*) and scalar (s_*), and among the vector ones the popcounts and funnel shifts."""
import re
import sys


def main(path):
    lines = open(path).read().splitlines()
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_ZN\S*read_overlaps_kernel[^ ]*:", l)]
    for i, name in starts:
        words, iupac = re.search(r"ILi(\d+)ELb(\d)E", name).groups()
        end = next(j for j in range(i, len(lines)) if "s_endpgm" in lines[j])
        body = lines[i:end]
        labels = {m.group(1): j for j, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
        best = None
        for j, l in enumerate(body):
            m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
            if m and labels.get(m.group(1), 1 << 30) < j:
                blk = [x.strip() for x in body[labels[m.group(1)]:j + 1] if x.strip() and not x.strip().startswith((".", ";"))]
                if any("bcnt" in x for x in blk) and (best is None or len(blk) > len(best)):
                    best = blk
        v = [x for x in best if x.startswith("v_")]
        print(f"words={words} {'iupac' if iupac == '1' else 'dna'}: round loop {len(best)} instructions, VALU {len(v)} (popcount {sum('bcnt' in x for x in v)}, "
              f"funnel shift {sum('alignbit' in x for x in v)}), LDS {sum(x.startswith('ds_') for x in best)}, scalar {sum(x.startswith('s_') for x in best)}")


if __name__ == "__main__":
    main(sys.argv[1])
