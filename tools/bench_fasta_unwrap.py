"""The FASTA unwrap on the device next to the host unwrap it replaces, over the same bytes: a seeded synthetic genome FASTA
(24 records of unequal length, 60 bases per line, 2 % N in runs).  The legs alternate inside one repetition loop after a
warm-up, so that they see the same machine.  Run it in a fresh process.

    python tools/bench_fasta_unwrap.py [--bytes 1000000000] [--reps 7] [--out profiles/fasta_unwrap_bench.json]

  host     (a) the yardstick: fastx._parse_chunk on the chunk's bytes (the numpy unwrap) + the upload of the unwrapped text
  device   (b) sassy_hip_fasta_unwrap on the host bytes: the upload of the raw bytes + the three passes
  resident (c) sassy_hip_fasta_unwrap on device-resident raw bytes, by device events around the call: the kernel sequence with
           its two host waits and its allocations, no upload

Per leg the median, min, max and (max - min) / median of the repetitions.  For (c) the bytes the three passes must move are
computed here from the shapes -- the raw bytes twice, the kept bytes and pads once, a 16-byte entry per 4 KiB tile written
once and read twice, the record arrays -- and divided by the time and by the HBM peak: a kernel-SEQUENCE share (launch gaps,
host waits and hipMalloc included), not a kernel's.  The warm-up compares the device's records with the host's, byte for byte.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes / s (spec); about 6.3e12 is what streaming kernels reach
N_RECORDS, WIDTH = 24, 60


def summary(v):
    med = statistics.median(v)
    return {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4), "spread": round((max(v) - min(v)) / med, 4) if med else 0.0}


def synthetic_fasta(total: int, seed: int):
    """About `total` bytes of FASTA as a numpy uint8 array."""
    import numpy as np
    rng = np.random.default_rng(seed)
    weights = rng.uniform(0.2, 1.0, N_RECORDS)
    lens = np.maximum(1, (weights / weights.sum() * total * WIDTH / (WIDTH + 1)).astype(np.int64))
    parts = []
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for r, n in enumerate(lens):
        n = int(n)
        seq = acgt[rng.integers(0, 4, size=n, dtype=np.uint8)]
        for at in rng.integers(0, max(1, n - 1000), size=max(1, n // 50000)):  # 2 % N in runs of 1000
            seq[int(at):int(at) + 1000] = ord("N")
        rows = n // WIDTH
        body = np.empty(rows * (WIDTH + 1), dtype=np.uint8)
        grid = body.reshape(rows, WIDTH + 1)
        grid[:, :WIDTH] = seq[:rows * WIDTH].reshape(rows, WIDTH)
        grid[:, WIDTH] = 10
        parts += [np.frombuffer(b">chr%d synthetic record %d of %d\n" % (r + 1, r + 1, N_RECORDS), dtype=np.uint8), body]
        if n % WIDTH:
            parts += [seq[rows * WIDTH:], np.frombuffer(b"\n", dtype=np.uint8)]
    return np.concatenate(parts)


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


def bytes_moved(n: int, fa) -> dict:
    tiles = (n + 4095) // 4096
    kept = int(fa.seq_lens.sum())
    records = len(fa)
    read = 2 * n + 2 * 16 * tiles + records * (3 * 8 * 2 + 32)      # raw twice; tile entries twice; record arrays, table
    written = fa.text_bytes + 16 * tiles + records * (3 * 8 + 32)    # kept bytes, pads and spare; tile entries; record arrays, table
    return {"read": read, "written": written, "total": read + written, "kept": kept, "tiles": tiles, "records": records}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_unwrap_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import sassy_amd
    from sassy_amd import fastx
    if sassy_amd.device_count() == 0:
        raise SystemExit("no HIP device visible: nothing is measured without one")
    t0 = time.perf_counter()
    made = synthetic_fasta(a.bytes, a.seed)
    n = int(made.size)
    raw_map, raw = fastx._big(n)  # (the reader's own kind of buffer: anonymous memory, huge pages asked for)
    raw = raw[:n]
    raw[:] = made
    del made
    print(f"input: {n} bytes, {N_RECORDS} records, made in {time.perf_counter() - t0:.1f} s", flush=True)
    work = fastx._Work()
    d_raw = sassy_amd.DeviceBuffer((n + 63) // 64 * 64)
    sassy_amd._check(sassy_amd.lib().sassy_hip_memcpy_h2d(d_raw.ptr, raw.ctypes.data, n))
    resident = sassy_amd.DeviceText(d_raw.ptr, n, owner=d_raw)
    d_host_text = sassy_amd.DeviceBuffer(n)  # where leg (a) uploads its unwrapped text
    events = Events()

    def leg_host():
        t = time.perf_counter()
        rb = fastx._parse_chunk(raw, False, work, raw_map)
        buf = rb.texts.buffer
        sassy_amd._check(sassy_amd.lib().sassy_hip_memcpy_h2d(d_host_text.ptr, buf.ctypes.data, buf.size))
        return (time.perf_counter() - t) * 1e3, rb

    def leg_device():
        t = time.perf_counter()
        fa = sassy_amd.DeviceFasta(raw)
        return (time.perf_counter() - t) * 1e3, fa

    def leg_resident():
        events.start()
        fa = sassy_amd.DeviceFasta(resident)
        return events.stop_ms(), fa

    # warm-up, and the check: same records, same bytes
    _, rb = leg_host()
    _, fa = leg_device()
    _, fr = leg_resident()
    assert len(fa) == len(fr) == len(rb) == N_RECORDS, (len(fa), len(fr), len(rb))
    for f in (fa, fr):
        assert (f.seq_lens == rb.texts.lens).all()
        for i in range(len(f)):
            assert f.id(i) == rb.id(i)
            step = 64 << 20
            for at in range(0, int(f.seq_lens[i]), step):
                assert f.download(i, at, at + step) == rb.sequence(i)[at:at + step], (i, at)
    moved = bytes_moved(n, fr)
    fa.free()
    fr.free()
    print("warm-up done, results equal", flush=True)

    ms = {"host": [], "device": [], "resident": []}
    for rep in range(a.reps):
        t, _ = leg_host()
        ms["host"].append(t)
        t, f = leg_device()
        f.free()
        ms["device"].append(t)
        t, f = leg_resident()
        f.free()
        ms["resident"].append(t)
        print(f"rep {rep}: host {ms['host'][-1]:.1f} ms, device {ms['device'][-1]:.1f} ms, resident {ms['resident'][-1]:.2f} ms", flush=True)

    res_s = statistics.median(ms["resident"]) / 1e3
    out = {
        "input": {"bytes": n, "records": N_RECORDS, "line_width": WIDTH, "seed": a.seed, "n_fraction": 0.02},
        "reps": a.reps,
        "host_unwrap_plus_upload_ms": summary(ms["host"]),
        "raw_upload_plus_device_unwrap_ms": summary(ms["device"]),
        "device_unwrap_resident_ms": summary(ms["resident"]),
        "device_over_host": round(statistics.median(ms["host"]) / statistics.median(ms["device"]), 3),
        "input_gb_per_s": {k: round(n / 1e9 / (statistics.median(v) / 1e3), 3) for k, v in ms.items()},
        "resident_bytes_moved": moved,
        "resident_sequence_bytes_per_s": round(moved["total"] / res_s, 1),
        "resident_sequence_share_of_hbm_peak": round(moved["total"] / res_s / HBM_PEAK, 4),
        "hbm_peak_bytes_per_s": HBM_PEAK,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
