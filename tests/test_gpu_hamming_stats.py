"""GPU: every call of tests/golden/hamming_stats.json leaves the stats() it left when the table was recorded
(tools/record_hamming_stats.py; the commit is named in the file) -- all fields but the times -- and returns as many records."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import hamming_stats  # noqa: E402

pytestmark = pytest.mark.gpu

ENTRIES = ("search_hamming", "hamming_counts", "search_hamming_many", "hamming_best_pattern", "hamming_counts_many", "hamming_amplicons")


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "hamming_stats.json")))
    recorded = [{k: v for k, v in c.items() if k != "stats"} for c in g["calls"]]
    assert recorded == hamming_stats.calls() and g["text_bytes"] == hamming_stats.TEXT_BYTES  # the table is of these calls
    return g


@pytest.fixture(scope="module")
def base():
    return hamming_stats.texts()


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_recorded_call_leaves_its_recorded_stats(entry, golden, base):
    """One fresh Searcher per call over a text of three tiles and a partial one (the batch calls: texts of 4000, 0 and 4100
    bytes): patterns of 1, 64, 65 and 130 rows alone and together, k 0 and 2, one strand and two, two Ascii patterns that share
    no slot; default options, and hamming_items=64 / hamming_records=7 / hamming_batch=1, which force list overflows, several
    record batches and one pattern per launch; the batch calls also with hamming_many_batch 8192 and 4096.  Measured when
    recording: 167 calls in 5.5 s, 33 ms a call (a fresh searcher and its first search); at most 42 calls per entry point."""
    sys.path.insert(0, ROOT)
    import sassy_amd
    assert sassy_amd.device_count() > 0
    calls = [c for c in golden["calls"] if c["entry"] == entry]
    assert calls
    wrong = []
    for call in calls:
        got = hamming_stats.run_call(sassy_amd, base, call)
        assert not any(name.endswith("_ms") for name in got)
        if got != call["stats"]:
            wrong.append(({k: v for k, v in call.items() if k != "stats"},
                          {name: (call["stats"].get(name), got.get(name)) for name in set(got) | set(call["stats"]) if call["stats"].get(name) != got.get(name)}))
    assert not wrong, (len(wrong), wrong[:5])
