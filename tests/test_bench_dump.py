"""CPU-only tests of bench.py --dump-outputs: the Match records of the last timed search as float .npy files, the same
from a sassy_amd.Result (N = 1) and from the merged rows of the rank path (N > 1), at most 64 MB in all."""
import glob
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import sassy_amd  # noqa: E402
from sassy_amd import multigpu  # noqa: E402


def fake_result(text_start, cigars):
    """A stand-in for sassy_amd.Result: the numpy records (include/sassy_hip.h: sassy_hip_Match) and the cigar pool."""
    n = len(cigars)
    a = np.zeros(n, dtype=sassy_amd.match_dtype())
    a["text_start"] = text_start
    a["text_end"] = a["text_start"] + 32
    a["pattern_end"] = 32
    a["cost"] = np.arange(n) % 4
    a["strand"] = np.arange(n) % 2
    a["cigar_len"] = [len(c) for c in cigars]
    a["cigar_off"] = np.concatenate([[0], np.cumsum(a["cigar_len"])[:-1]]) if n else []
    return types.SimpleNamespace(array=a, pool=b"".join(cigars), exit_state=multigpu.STATE_PASS, conditional_index=-1)


def load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(d, "*.npy"))}


def test_dump_of_a_result_equals_the_dump_of_rank_rows(tmp_path):
    cigars = [b"32=", b"10=1X21=", b"5=1I26=", b"", b"31=1D1="]
    r = fake_result([10, 20, 3_000_000_001, 40, 50], cigars)
    bench.dump_outputs(str(tmp_path / "one"), r)
    bench.dump_outputs(str(tmp_path / "ranks"), multigpu.pack_result_numpy(r, cigar_bytes=24).rows)
    one, ranks = load(tmp_path / "one"), load(tmp_path / "ranks")
    assert sorted(one) == sorted(bench.DUMP_FIELDS + ("cigar", "row"))
    for name, x in one.items():
        assert x.dtype == (np.float32 if name == "cigar" else np.float64), name
        assert np.array_equal(x, ranks[name]), name
    assert one["text_start"][2] == 3_000_000_001 and list(one["row"]) == [0, 1, 2, 3, 4]
    assert list(one["strand"]) == [0, 1, 0, 1, 0] and list(one["cost"]) == [0, 1, 2, 3, 0]
    assert [bytes(c.astype(np.uint8)).rstrip(b"\0") for c in one["cigar"]] == cigars


def test_dump_of_an_empty_result(tmp_path):
    bench.dump_outputs(str(tmp_path), fake_result([], []))
    got = load(tmp_path)
    assert got["cigar"].shape == (0, 0) and all(got[f].shape == (0,) for f in bench.DUMP_FIELDS + ("row",))


def test_dump_of_a_large_result_is_a_fixed_sample_under_64_mb(tmp_path):
    n = 1_500_000
    r = fake_result(np.arange(n) * 7, [b"32="] * n)
    bench.dump_outputs(str(tmp_path / "a"), r)
    bench.dump_outputs(str(tmp_path / "b"), r)
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))) <= 64_000_000
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    rows = a["row"]
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(a["text_start"], rows * 7)
