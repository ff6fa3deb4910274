"""CPU-only: the route of a scan job (sassy_amd/csrc/scan_route.h), driven by a stand-alone host program
(tests/c/scan_route_driver.cc: its own main, no HIP call, never loaded into Python) built with the host compiler under
AddressSanitizer / UBSan -- the routes recorded in tests/golden/scan_routes.json, what every route keeps, and the filter's
launch parameters and tables against brute force."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


def _rocm_include():
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "/opt/rocm/include"):
        if os.path.isdir(os.path.join(d, "hip")):
            return d
    raise AssertionError("no ROCm include directory")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("scan_route") / "scan_route_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "c", "scan_route_driver.cc")])
    return exe


def test_route_header_is_host_only():
    src = open(os.path.join(CSRC, "scan_route.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert [i for i in includes if i.startswith('"')] == ['"profiles.h"', '"switches.h"']
    assert "hipStream" not in src and "hipMemcpy" not in src and "__global__" not in src and "L.upload" not in src
    # one owner: the driver keeps none of what moved
    drv = open(os.path.join(CSRC, "scan_driver.hip")).read()
    for name in ("filter_piece_len", "pair_geometry", "plain_prefix", "clumped_tail", "build_qgram_table", "build_count_table"):
        assert name + "(" in src and name not in drv, name
    assert "pair_eligible(" in src and drv.count("pair_eligible(") == 1  # search_text() asks the header


def _class_slots(sassy, alphabet, expr):
    cp = sassy.parse_classes(expr)
    sets = set()
    for j in range(cp.m):
        members = set(cp.members(j))
        if alphabet == "ascii_ci":
            members |= {c ^ 0x20 for c in members if chr(c).isalpha() and c < 128}
        sets.add(frozenset(members))
    return cp.m, len(sets)


def _driver_line(sassy, row):
    opts = dict(row["opts"])
    prefilter = opts.pop("prefilter", -1)
    fuse = opts.pop("fused", 1)
    trace = opts.pop("trace", 1)
    if row.get("classes"):
        m, nslots = _class_slots(sassy, row["alphabet"], row["pattern"].encode("latin-1"))
        hexpat = "-"
    else:
        m, nslots, hexpat = len(row["pattern"]), 0, row["pattern"].encode("latin-1").hex()
    words = [row["alphabet"], int(row["rc"]), int(row["alpha"] is not None), trace, prefilter, fuse, int(bool(row.get("classes"))), m, nslots,
             row["k"], len(opts)]
    for name, value in opts.items():
        words += [name, value]
    return " ".join(str(w) for w in words + [hexpat])


def test_golden_rows_take_the_recorded_route(driver):
    """Every row of tests/golden/scan_routes.json through choose_route(): (filtered ? kind : 0, piece length, fused,
    fused ? pair : 0) as recorded on a device.  A row with rc: the two or three jobs search_text() runs, the last one's route.
    Rows that cannot be named this way are skipped and counted; none with rc = False may be."""
    sys.path.insert(0, ROOT)
    import sassy_amd
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "scan_routes.json")))
    rows = golden["rows"]
    covered = list(rows)  # (every row can be named: both strands are the driver's rows mode)
    skipped = len(rows) - len(covered)
    print("rows", len(rows), "skipped", skipped, "skipped with rc = False", sum(1 for r in rows if r not in covered and not r["rc"]))
    assert not [r for r in rows if not r["rc"] and r not in covered]
    text = "\n".join(_driver_line(sassy_amd, r) for r in covered) + "\n"
    p = subprocess.run([driver, "rows"], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]
    assert len(got) == len(covered)
    wrong = [(r, g) for r, g in zip(covered, got) if g != r["stats"][:4]]
    assert not wrong, (len(wrong), wrong[:5])
    # the sweep reaches every filter kind, the streaming DP, the paired and the fused launch, both ways
    seen = {tuple(r["stats"][:1]) for r in rows}
    assert {(0,), (1,), (2,), (3,), (4,)} <= seen
    assert {r["stats"][2] for r in rows} == {0, 1} and {r["stats"][3] != 0 for r in rows} == {False, True}


def test_route_invariants_hold_for_every_shape(driver):
    """profile x m in [1, 130] x k in [0, 16] x pattern kind x option, without ext_bitmap / ext_desc: the driver exits
    non-zero on the first route that breaks one of the invariants (among them: an Iupac bit-plane filter is fused -- the
    condition ScanJob::prepare() used to fail on)."""
    p = subprocess.run([driver, "invariants"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout + p.stderr[-3000:]
    f = {k: int(v) for k, v in (kv.split("=") for kv in p.stdout.split()[1:])}
    assert f["routes"] > 500_000 and f["none"] + f["generic"] + f["planes"] + f["table"] + f["count"] == f["routes"]
    assert min(f["generic"], f["planes"], f["table"], f["count"], f["pair"], f["fused"], f["direct"]) > 100


def test_packing_and_tables_against_brute_force(driver):
    for seed in ("1", "2"):
        p = subprocess.run([driver, "packing", seed], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.strip() == "ok packed=400 tables=96", p.stdout + p.stderr[-3000:]
