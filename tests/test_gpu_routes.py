"""GPU: every search of tests/golden/scan_routes.json takes the route it took when the table was recorded
(tools/record_scan_routes.py; the commit is named in the file) and finds as many matches."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import scan_routes  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_recorded_search_takes_its_recorded_route():
    """One fresh Searcher and one search of a 64 KiB text per row; filtered, piece_len, fused, pair of stats() and the number
    of matches are the recorded ones.  Measured when recording, on the recorded commit: 1542 rows in 32.9 s, 21 ms a row (a
    fresh searcher and its first search); the option cross-product was then cut to the 407 rows kept, 8.7 s of that."""
    sys.path.insert(0, ROOT)
    import sassy_amd
    assert sassy_amd.device_count() > 0
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "scan_routes.json")))
    base = scan_routes.texts()
    assert golden["text_bytes"] == len(base["dna"]) == len(base["prose"])
    wrong = []
    for row in golden["rows"]:
        got = scan_routes.run_row(sassy_amd, base, row)
        if got != row["stats"]:
            wrong.append(({k: v for k, v in row.items() if k != "stats"}, row["stats"], got))
    assert not wrong, (len(wrong), wrong[:5])
