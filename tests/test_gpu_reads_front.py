"""The front of the read-batch calls on the device against tests/golden/reads_front.json, recorded on the commit before the calls
got one owner for their refusals and their frame (tools/record_reads_front.py; the calls are tests/helpers/reads_front.py's):
code and full message of every refusal that reads a handle -- too long, parsed without kept quality, counts differ, null out
behind the handle, searches in flight, another device where there are two --, the stats after each of the calls and after a
failed one, for batches of 0, 1 and 5 reads of at most 40 bytes.  Every comparison is exact equality.  Each returned batch,
downloaded, equals what reads_slice / reads_select make of the same windows."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, ROOT)

import reads_front  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


@pytest.fixture(scope="module")
def replay(sassy):
    return reads_front.device(sassy)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "reads_front.json")))["device"]


def _compare(got, want):
    want = {e["call"]: e for e in want}
    assert len({e["call"] for e in got}) == len(got)
    for e in got:
        assert e["call"] in want, ("the golden file lacks", e["call"])
        assert e == want[e["call"]], (e, want[e["call"]])


def test_refusals_that_read_a_handle_are_the_recorded_ones(replay, golden):
    got = replay["refusals"]
    _compare(got, golden["refusals"])
    assert len(got) >= 2 * (6 * 3 + 12) + 6 * 3
    for word in ("takes reads of at most 512 bytes", "the longest are 513 and 513", "the longest has 513", "was parsed without SASSY_HIP_KEEP_QUALITY",
                 "were parsed without SASSY_HIP_KEEP_QUALITY", "r1 holds 2 reads, r2 holds 3", "must not be null (out_merged)", "must not be null (out_trimmed)",
                 "must not be null (out_bounds, out_sorted)", "must not be null (out_dedup)", "must not be null (out_label)", "finish them first"):
        assert any(word in e["msg"] for e in got), word
    assert sum("finish them first" in e["msg"] for e in got) == 6


def test_stats_and_returned_batches_are_the_recorded_ones(replay, golden):
    got = replay["stats"]
    _compare(got, golden["stats"])
    assert len(got) == 2 * (3 * 9 + 10)
    # what the dna searcher refuses after its look at the batch, and before it for an adapter or a barcode
    errors = [e for e in got if "error" in e]
    assert len(errors) == 9 and all(e["call"].startswith("dna N ") and "use an iupac searcher" in e["error"] for e in errors)
    # every call that returns a batch returned the windows of its source
    checked = [e for e in got if "same" in e]
    assert len(checked) == 2 * 3 * 7 and all(e["same"] is True and e["stats_after_windows"] == e["stats"] for e in checked)
    ran = {e["call"]: e["stats"] for e in got if "error" not in e}
    assert ran["dna n=5 trim_reads"]["scan_launches"] == 6 and ran["iupac n=5 trim_reads"]["scan_launches"] == 5       # the look is counted ...
    assert ran["dna n=5 read_overlaps"]["scan_launches"] == ran["iupac n=5 read_overlaps"]["scan_launches"] == 1         # ... or not, as before
    assert ran["dna n=5 dedup_reads no window"] == dict(ran["dna n=0 dedup_reads"], filtered=12) and ran["dna n=0 dedup_reads"]["scan_launches"] == 0
