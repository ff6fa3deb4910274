"""Text-pass occupancy of a stream of searches from a rocprofv3 --kernel-trace CSV: the filter dispatches of the last
N searches (filter_dna_kernel, lone or grouped, whole or a workgroup range), their durations by shape, and how long the
device had no filter dispatch running between the first and the last of them (the idle share of a step).
Usage: python tools/pass_idle.py <dir with *kernel_trace.csv> [searches, default 200]"""
import csv, glob, os, re, sys
from collections import defaultdict

root = sys.argv[1]
want = int(sys.argv[2]) if len(sys.argv) > 2 else 200
rows = []
for f in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
    with open(f) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"]
            if "filter_dna_kernel" not in name:
                continue
            m = re.search(r"filter_dna_kernel<([^>]*)>", name)
            args = [a.strip() for a in m.group(1).split(",")] if m else []
            members = 2 if len(args) >= 7 and args[6] == "2" else 1
            grid = int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0) // max(1, int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 256)) or 256))
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), members, grid))
rows.sort()
if not rows:
    sys.exit("no filter_dna_kernel dispatch in " + root)
whole = max(g for _, _, _, g in rows)
# walk back from the end until the dispatches cover `want` searches (a dispatch over a part of the grid serves that part)
served, i = 0.0, len(rows)
while i > 0 and served < want:
    i -= 1
    served += rows[i][2] * rows[i][3] / whole
win = rows[i:]
t0, t1 = win[0][0], max(e for _, e, _, _ in win)
busy, cur_s, cur_e = 0, win[0][0], win[0][1]
gaps = []
for s, e, _, _ in win[1:]:
    if s > cur_e:
        busy += cur_e - cur_s
        gaps.append(s - cur_e)
        cur_s, cur_e = s, e
    else:
        cur_e = max(cur_e, e)
busy += cur_e - cur_s
span = t1 - t0
by = defaultdict(list)
for s, e, m, g in win:
    by[(m, g)].append(e - s)
print(f"{len(win)} filter dispatches serve {served:.1f} searches in {span / 1e6:.3f} ms: {span / served / 1e6:.4f} ms per search")
for (m, g), v in sorted(by.items()):
    v.sort()
    print(f"  members {m} workgroups {g:5d}: n={len(v):4d} median {v[len(v) // 2] / 1e6:.4f} ms  min {v[0] / 1e6:.4f}  max {v[-1] / 1e6:.4f}  sum {sum(v) / 1e6:.3f} ms")
print(f"  no filter dispatch running: {(span - busy) / 1e6:.3f} ms = {100.0 * (span - busy) / span:.1f} % of the window, {(span - busy) / served / 1e6:.4f} ms per search"
      f" ({len(gaps)} gaps, median {sorted(gaps)[len(gaps) // 2] / 1e6 if gaps else 0:.4f} ms)")
