"""Demultiplexing a FASTQ file with the parse on the host (the path before sassy_hip_fastq_parse) and on the device, over the
same seeded synthetic reads: 150 bases, 96 barcodes of 16-24 bases planted with 0-2 substitutions on either strand, k = 2,
Dna, both strands.  The legs alternate inside one repetition loop after a warm-up, so that they see the same machine.  Run it
in a fresh process.

    python tools/bench_fastq_reads.py [--reads 100000 3200000] [--reps 5] [--out profiles/fastq_reads_bench.json]

  host_path    (a) fastx.read_fastx_batches over the file + Searcher.hamming_best_pattern on the host texts of every batch:
               numpy line table, layout into pinned memory, upload of the laid-out batch, scan
  device_path  (b) fastx.read_fastq_device_batches over the file + hamming_best_pattern on the resident batch: upload of the
               raw bytes, sassy_hip_fastq_parse, scan (sassy_hip_hamming_best_pattern_reads); the ids are copied out per batch
  parse        (c) sassy_hip_fastq_parse alone on device-resident raw bytes of the whole file, by device events around the
               call: the kernel sequence with its host waits and allocations, no upload
  scan_reads / scan_host   (d) hamming_best_pattern on the resident batch of the whole file, and on the host texts of the same
               reads (one call each; the host call lays out and uploads, which is what the resident one saves)

(a) and (b) read the same file in batches of --batch-bytes, as `demux` does without and with --device-parse (the rows it
formats are left out of both).  Per leg the median, min, max and (max - min) / median of the repetitions.  For (c) the bytes
the passes must move are computed here from the shapes -- the raw bytes twice, the sequence bytes once more, the text once,
eight bytes and a flag per line written once and read by the record and copy passes -- and divided by the time and by the HBM
peak: a kernel-SEQUENCE share (launch gaps, host waits and hipMalloc included), not a kernel's.  The warm-up compares the two
paths' results.  Besides the JSON the run writes the figures of DESIGN.md 5.8b as a table next to it (.md)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s (spec)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ_LEN = 150


def summary(v):
    med = statistics.median(v)
    return {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4), "spread": round((max(v) - min(v)) / med, 4) if med else 0.0}


def synthetic_fastq(n_reads: int, seed: int):
    """(barcodes, raw uint8 array): rows of '@read' + 9 digits, 150 bases, '+', 150 quality bytes."""
    import numpy as np
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    barcodes = [letters[rng.integers(0, 4, int(rng.integers(16, 25)))].tobytes() for _ in range(96)]
    reads = letters[rng.integers(0, 4, (n_reads, READ_LEN), dtype=np.uint8)]
    which, minus = rng.integers(0, 96, n_reads), rng.integers(0, 2, n_reads).astype(bool)
    for b, bc in enumerate(barcodes):
        for strand in (False, True):
            rows = np.flatnonzero((which == b) & (minus == strand))
            w = np.frombuffer(bc.translate(COMP)[::-1] if strand else bc, dtype=np.uint8)
            win = np.tile(w, (rows.size, 1))
            for _ in range(2):  # up to two substitutions (one that draws the same letter is none)
                hit = rng.integers(0, 3, rows.size) > 0
                win[hit, rng.integers(0, len(w), int(hit.sum()))] = letters[rng.integers(0, 4, int(hit.sum()))]
            at = rng.integers(0, READ_LEN - len(w) + 1, rows.size)
            reads[rows[:, None], at[:, None] + np.arange(len(w))[None, :]] = win
    head = 5 + 9 + 1
    row = head + READ_LEN + 3 + READ_LEN + 1
    grid = np.empty((n_reads, row), dtype=np.uint8)
    grid[:, :5] = np.frombuffer(b"@read", dtype=np.uint8)
    digits = np.arange(n_reads, dtype=np.int64)
    for d in range(9):
        grid[:, 5 + 8 - d] = ord("0") + digits % 10
        digits //= 10
    grid[:, head - 1] = 10
    grid[:, head:head + READ_LEN] = reads
    grid[:, head + READ_LEN:head + READ_LEN + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    grid[:, head + READ_LEN + 3:row - 1] = ord("I")
    grid[:, row - 1] = 10
    return barcodes, grid.reshape(-1)


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


def bytes_moved(n: int, reads) -> dict:
    tiles, lines, records = (n + 4095) // 4096, 4 * len(reads), len(reads)
    seq = int(reads.seq_lens.sum())
    blocks = (reads.text_bytes - 64) // 64
    # raw twice (count, lines) and the sequences once more (copy); tile counts; per line start and flag by the record passes
    # (twice: sum and write) and the sequence's start by the copy; the start table by the copy's search
    read = 2 * n + seq + 2 * 4 * tiles + 2 * 9 * lines + 8 * records + 16 * blocks
    written = reads.text_bytes + 4 * blocks + 4 * tiles + 9 * lines + records * (48 + 16)
    return {"read": read, "written": written, "total": read + written, "sequence_bytes": seq, "text_bytes": reads.text_bytes, "records": records}


def run_size(sassy_amd, n_reads, a, tmp):
    import numpy as np
    from sassy_amd import fastx
    t0 = time.perf_counter()
    barcodes, raw = synthetic_fastq(n_reads, a.seed)
    n = int(raw.size)
    path = os.path.join(tmp, f"reads_{n_reads}.fq")
    raw.tofile(path)
    print(f"{n_reads} reads: {n} bytes of FASTQ, made and written in {time.perf_counter() - t0:.1f} s", flush=True)
    s = sassy_amd.Searcher("dna", rc=True)
    events = Events()
    d_raw = sassy_amd.DeviceBuffer((n + 63) // 64 * 64)
    sassy_amd._check(sassy_amd.lib().sassy_hip_memcpy_h2d(d_raw.ptr, raw.ctypes.data, n))
    resident_raw = sassy_amd.DeviceText(d_raw.ptr, n, owner=d_raw)
    host_batch = fastx._parse_single_line_records(raw, 4).texts

    def host_path():
        t, out = time.perf_counter(), []
        for batch in fastx.read_fastx_batches(path, a.batch_bytes):
            out.append(s.hamming_best_pattern(barcodes, batch.texts, a.k))
        return (time.perf_counter() - t) * 1e3, out

    def device_path():
        t, out = time.perf_counter(), []
        for batch in fastx.read_fastq_device_batches(path, a.batch_bytes):
            out.append(s.hamming_best_pattern(barcodes, batch.texts, a.k))
            batch.free()
        return (time.perf_counter() - t) * 1e3, out

    def parse():
        events.start()
        reads = sassy_amd.DeviceReads(resident_raw)
        return events.stop_ms(), reads

    def scan_reads(reads):
        t = time.perf_counter()
        out = s.hamming_best_pattern(barcodes, reads, a.k)
        return (time.perf_counter() - t) * 1e3, out

    def scan_host():
        t = time.perf_counter()
        out = s.hamming_best_pattern(barcodes, host_batch, a.k)
        return (time.perf_counter() - t) * 1e3, out

    # warm-up, and the check: the same answer per read on both paths and from both scans
    _, want = host_path()
    _, got = device_path()
    want = [np.concatenate([b[i] for b in want]) for i in range(4)]
    got = [np.concatenate([b[i] for b in got]) for i in range(4)]
    assert all(np.array_equal(x, y) for x, y in zip(want, got)) and len(want[0]) == n_reads
    _, reads = parse()
    assert len(reads) == n_reads and all(np.array_equal(x, y) for x, y in zip(scan_reads(reads)[1], want))
    assert all(np.array_equal(x, y) for x, y in zip(scan_host()[1], want))
    moved = bytes_moved(n, reads)
    assigned = int((want[0] != sassy_amd.NO_MATCH).sum())
    print(f"warm-up done, results equal; {assigned} of {n_reads} reads assigned", flush=True)

    ms = {"host_path": [], "device_path": [], "parse": [], "scan_reads": [], "scan_host": []}
    for rep in range(a.reps):
        ms["host_path"].append(host_path()[0])
        ms["device_path"].append(device_path()[0])
        t, fresh = parse()
        fresh.free()
        ms["parse"].append(t)
        ms["scan_reads"].append(scan_reads(reads)[0])
        ms["scan_host"].append(scan_host()[0])
        print(f"rep {rep}: " + ", ".join(f"{k} {v[-1]:.2f} ms" for k, v in ms.items()), flush=True)
    reads.free()
    d_raw.free()
    os.remove(path)
    parse_s = statistics.median(ms["parse"]) / 1e3
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {
        "input": {"reads": n_reads, "read_len": READ_LEN, "raw_bytes": n, "sequence_bytes": moved["sequence_bytes"], "laid_out_bytes": moved["text_bytes"],
                  "raw_over_sequence": round(n / moved["sequence_bytes"], 3), "laid_out_over_sequence": round(moved["text_bytes"] / moved["sequence_bytes"], 3),
                  "barcodes": len(barcodes), "k": a.k, "assigned": assigned, "batch_bytes": a.batch_bytes, "seed": a.seed},
        "ms": {k: summary(v) for k, v in ms.items()},
        "host_over_device_path": round(med["host_path"] / med["device_path"], 3),
        "paths_differ_beyond_both_spreads": bool(min(ms["host_path"]) > max(ms["device_path"]) or min(ms["device_path"]) > max(ms["host_path"])),
        "scan_host_over_scan_reads": round(med["scan_host"] / med["scan_reads"], 3),
        "parse_bytes_moved": moved,
        "parse_raw_gb_per_s": round(n / 1e9 / parse_s, 3),
        "parse_bytes_per_s": round(moved["total"] / parse_s, 1),
        "parse_share_of_hbm_peak": round(moved["total"] / parse_s / HBM_PEAK, 4),
    }


def markdown(out) -> str:
    rows = ["| reads | raw bytes | (a) host path | (b) device path | (a) / (b) | (c) parse, resident | (d) scan, resident | (d) scan, host texts |",
            "|---|---|---|---|---|---|---|---|"]
    cell = lambda v: f"{v['median']:.1f} ms ({v['min']:.1f} .. {v['max']:.1f})"  # noqa: E731
    for r in out["sizes"]:
        m = r["ms"]
        rows.append(f"| {r['input']['reads']} | {r['input']['raw_bytes']} | {cell(m['host_path'])} | {cell(m['device_path'])} | "
                    f"{r['host_over_device_path']} | {cell(m['parse'])}, {r['parse_raw_gb_per_s']} GB/s of raw | {cell(m['scan_reads'])} | "
                    f"{cell(m['scan_host'])} |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[100_000, 3_200_000])  # 3.2 M reads: 1.0 GB of raw bytes
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("-k", type=int, default=2)
    ap.add_argument("--batch-bytes", type=int, default=64 << 20)  # cli.BATCH_BYTES
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_reads_bench.json"))
    a = ap.parse_args()
    import sassy_amd
    if sassy_amd.device_count() == 0:
        raise SystemExit("no HIP device visible: nothing is measured without one")
    out = {"reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK, "sizes": []}
    with tempfile.TemporaryDirectory() as tmp:
        for n_reads in a.reads:
            out["sizes"].append(run_size(sassy_amd, n_reads, a, tmp))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    with open(os.path.splitext(a.out)[0] + ".md", "w") as fh:
        fh.write(markdown(out))
    print(json.dumps(out))
    print(markdown(out))


if __name__ == "__main__":
    main()
