"""CPU-only: the surface of the UMI grouping call (sassy_hip_umi_groups, Searcher.umi_groups, `cluster --umi`) -- what needs
no device: the symbol, every refusal with its code and message before any device work, the loud failure without a device,
the duplicate table of collapse_step.h and the directional rule of umi_step.h driven by stand-alone host programs under
AddressSanitizer / UBSan and under ThreadSanitizer, the source layout, the helper on a hand-written case, the CLI's parser and
row writer."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import umi_groups_ref as uref  # noqa: E402

NAME = "sassy_hip_umi_groups"
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


@pytest.fixture(scope="module")
def sassy():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


def test_symbol_is_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    L = sassy.lib()
    assert re.search(r"\b" + NAME + r"\s*\(", hdr)
    assert hasattr(L, NAME) and NAME in sassy.EXPORTED_SYMBOLS
    assert re.search(r"fn\s+" + NAME + r"\s*\(", block) and re.search(r"pub fn\s+umi_groups\s*\(", rust)
    assert getattr(L, NAME).restype is not None and len(getattr(L, NAME).argtypes) == 13
    assert hasattr(sassy.Searcher, "umi_groups") and sassy.UMI_METHODS == {"unique": 0, "cluster": 1, "directional": 2}
    for name, value in (("UNIQUE", 0), ("CLUSTER", 1), ("DIRECTIONAL", 2)):
        assert re.search(r"#define SASSY_HIP_UMI_%s\s+%du\b" % (name, value), hdr), name
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"umi_groups.hip"' in build and '"collapse_step.h"' in build and '"umi_step.h"' in build
    assert re.search(r"\b12: sassy_hip_umi_groups", hdr)
    # what the encoding folds is stated per profile
    doc = hdr[hdr.index("/* UMI grouping"):hdr.index("int " + NAME)]
    for word in ("Dna:", "Iupac:", "Ascii:", "ascii_ci:", "N and A MATCH but are no duplicates"):
        assert word in doc, word
    assert "collapse_slots" in [row[0] for row in sassy.option_table()]


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal with its code and a message that names the reason, in a child that sees no device: a call that got as far
    as the device would say 'no usable HIP device' instead.  Then valid arguments: that message."""
    code = r'''
import ctypes as C, numpy as np, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
A = b"ACGTACGT" + b"TTTTACGT"
def call(s, a=A, n=2, m=8, k=1, method=2, flags=0, out=True, s_null=False, optional=True):
    h = None if s_null else s._h
    cols = [np.zeros(16, dtype=np.uint32) for _ in range(4)]
    nu, ng = C.c_size_t(), C.c_size_t()
    opt = [c.ctypes.data if optional else None for c in cols[1:]]
    rc = L.sassy_hip_umi_groups(h, a, n, m, k, method, flags, cols[0].ctypes.data if out else None, opt[0], opt[1], opt[2],
                                C.byref(nu) if optional else None, C.byref(ng) if optional else None)
    return rc, L.sassy_hip_last_error().decode()
def refused(s, want, word, **kw):
    rc, msg = call(s, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (rc, msg, want, word)
dna = sassy_amd.Searcher("dna", rc=False)
# the family's own checks, through the pair calls' function
refused(sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang")
refused(sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match")
refused(sassy_amd.Searcher("ascii", rc=True), EUNSUPPORTED, "reverse complement is not defined")
refused(sassy_amd.Searcher("ascii_ci", rc=True), EUNSUPPORTED, "reverse complement is not defined")
refused(sassy_amd.Searcher("iupac", rc=True), EINVAL, "not valid IUPAC", a=b"ACGTACGT" + b"ACQTACGT")
refused(sassy_amd.Searcher("iupac", rc=True), EINVAL, "umi_groups: list a)", a=b"ACGTACGT" + b"ACQTACGT")
for alphabet in ("ascii", "ascii_ci"):
    refused(sassy_amd.Searcher(alphabet, rc=False), EUNSUPPORTED, "distinct bytes (pattern 1 has 65)", a=b"x" * 65 + bytes(range(128, 193)), m=65)
refused(sassy_amd.Searcher("dna", rc=False).with_max_n_frac(0.2), EUNSUPPORTED, "umi_groups does not take max_n_frac")
# the shape
refused(dna, EINVAL, "must be at least 1", m=0)
refused(dna, EINVAL, "must be <= 128", a=b"A" * 258, m=129)
refused(dna, EINVAL, "k must be <= 254", k=255)
refused(dna, EINVAL, "k must be <= 254", k=0x80000000)
refused(dna, EINVAL, "umi_groups needs at least one sequence", n=0)
for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.ALL_MINIMA, sassy_amd.TEXT_ON_DEVICE, sassy_amd.TEXT_UNCHANGED, sassy_amd.LINE_SPANS, 1 << 20):
    refused(dna, EINVAL, "umi_groups takes no flags", flags=flags)
refused(dna, EUNSUPPORTED, "2^31 - 1", n=1 << 31)
refused(dna, EINVAL, "umi_groups() must not be null", out=False)
refused(dna, EINVAL, "must not be null", a=None)
refused(dna, EINVAL, "must not be null", s_null=True)
# the method
for method in (3, 4, 0xFFFFFFFF):
    refused(dna, EINVAL, "unknown method %d" % method, method=method)
refused(dna, EINVAL, "k must be <= 254", k=255, method=0)   # (UNIQUE ignores k, the refusals do not)
# valid arguments get as far as the device: every method and alphabet, the limits themselves, the optional outputs left out
for s, kw in ((dna, {}), (dna, dict(method=0)), (dna, dict(method=1)), (dna, dict(optional=False)), (sassy_amd.Searcher("dna", rc=True), dict(k=254)),
              (sassy_amd.Searcher("iupac", rc=True), dict(a=b"ACGTNNRY" * 2)), (sassy_amd.Searcher("ascii", rc=False), {}),
              (sassy_amd.Searcher("ascii_ci", rc=False), dict(a=b"x" * 256, m=128)), (dna, dict(a=b"AC", m=1)), (dna, dict(n=1))):
    rc, msg = call(s, **kw)
    assert rc == ENODEVICE and "no usable HIP device" in msg, (rc, msg)
# the Python method: refusals of its own, then the same loud failure
for args, word in ((([b"ACGT", b"ACG"],), "sequence 1 has 3 bytes"), (([b"ACGT", sassy_amd.parse_classes(b"a[bc]")],), "ClassPattern"),
                   ((np.zeros((2, 4), dtype=np.int32),), "uint8 array"), ((np.zeros((4, 4), dtype=np.uint8)[:, ::2],), "C-contiguous"),
                   (([b"ACGT"], 300), "k must be <= 254"), (([],), "umi_groups needs at least one sequence"),
                   (([b"ACGT"], 1, "adjacency"), "method must be one of unique, cluster, directional"),
                   ((np.zeros((0, 4), dtype=np.uint8),), "needs at least one sequence"), (([b"ACGT", b"AAAA"],), "no usable HIP device"),
                   (([b"ACGT", b"AAAA"], 1, "unique"), "no usable HIP device"), (([b"ACGT", b"AAAA"], 1, "cluster"), "no usable HIP device"),
                   ((np.frombuffer(b"ACGTAAAA", dtype=np.uint8).reshape(2, 4), 1), "no usable HIP device")):
    try:
        dna.umi_groups(*args)
    except sassy_amd.SassyHipError as e:
        assert word in str(e), (word, e)
    else:
        raise SystemExit(3)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def _driver(tmp_path, name, sanitize, suffix=""):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / (name + suffix))
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all",
                           "-pthread", "-o", exe, os.path.join(ROOT, "tests", "c", name + ".cc")])
    return exe


def _run(exe, seed):
    r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    return {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}


def _check_collapse(fields):
    # 3 kinds x 8 sizes x 2 geometries x 3 hashes, each once from one thread and once from several; every entry inserted
    assert fields["tables"] == fields["threaded"] == 3 * 8 * 2 * 3
    assert fields["inserts"] == 3 * 2 * 3 * sum((1, 2, 3, 64, 65, 257, 1000, 4000))


def _check_relax(fields):
    assert fields["graphs"] == fields["threaded"] == 7 * 9 and fields["relaxes"] > 100000 and fields["longest"] >= 3


def test_duplicate_table_against_a_map_under_sanitizers(tmp_path):
    """tests/c/collapse_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: collapse_step.h with std::atomic on all-equal, all-distinct and mixed lists of up to 4000
    keys, tables at the default size and at load 1, the real hash and a hash forced to a constant, against a std::map --
    from one thread in three orders and from up to 8 threads."""
    exe = _driver(tmp_path, "collapse_step_driver", "address,undefined")
    for seed in ("1", "2"):
        _check_collapse(_run(exe, seed))


def test_duplicate_table_from_threads_under_thread_sanitizer(tmp_path):
    """The same program built with -fsanitize=thread: every access to the table is an atomic one."""
    _check_collapse(_run(_driver(tmp_path, "collapse_step_driver", "thread", "_tsan"), "3"))


def test_directional_rule_against_the_sequential_procedure_under_sanitizers(tmp_path):
    """tests/c/umi_step_driver.cc, -fsanitize=address,undefined: umi_step.h's relaxation to its fixpoint on paths, stars and
    random counted graphs of up to 4000 sequences against the sort / open / breadth-first procedure, within n + 1 passes; no
    label ever rises."""
    exe = _driver(tmp_path, "umi_step_driver", "address,undefined")
    for seed in ("1", "2", "3"):
        _check_relax(_run(exe, seed))


def test_directional_rule_from_threads_under_thread_sanitizer(tmp_path):
    exe = _driver(tmp_path, "umi_step_driver", "thread", "_tsan")
    for seed in ("4", "5"):
        _check_relax(_run(exe, seed))


def test_drivers_are_stand_alone_programs():
    for name, header in (("collapse_step_driver.cc", "collapse_step.h"), ("umi_step_driver.cc", "umi_step.h")):
        text = open(os.path.join(ROOT, "tests", "c", name)).read()
        assert "int main(" in text and "#include <hip" not in text and "__global__" not in text
        assert header in text and "std::atomic" in text and "std::thread" in text


def test_step_headers_stay_free_of_hip_and_state_their_rules():
    for name, functions, rules, operations in (
            ("collapse_step.h", ("collapse_hash", "collapse_slots_for", "collapse_insert", "collapse_lookup"),
             ("never returns to it", "ONE class", "whatever the hash", "no entry waits", "There is no spin", "plain look comes first"), {"load", "cas", "fetch_min"}),
            ("umi_step.h", ("umi_key", "umi_absorbs", "umi_jump", "umi_relax"),
             ("c_u >= 2 c_v - 1", "values only", "fixpoint", "Bellman-Ford", "n_u + 1 launches"), {"load", "fetch_min"})):
        src = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in src and "hipStream" not in src and "getenv" not in src, name
        assert "__builtin_amdgcn" not in src and "__HIP_DEVICE_COMPILE__" not in src and "asm" not in src, name
        for fn in functions:
            assert re.search(r"\b" + fn + r"\s*\(", src), fn
        for rule in rules:
            assert rule in src, (name, rule)
        code = "\n".join(line.split("//")[0] for line in src.splitlines())
        assert "__hip_atomic" not in code and set(re.findall(r"\bmem\.(\w+)\(", code)) == operations, name


def test_source_layout():
    """The entry point lives in umi_groups.hip; its refusals are the pair calls' function, called and not copied, and come
    before the device; it reaches the pair walk through the launchers of hamming_pairs.hip, whose kernels still exist once;
    the device policies are HIP's atomics at agent scope; no inline assembly, no environment."""
    unit = open(os.path.join(CSRC, "umi_groups.hip")).read()
    pairs = open(os.path.join(CSRC, "hamming_pairs.hip")).read()
    internal = open(os.path.join(CSRC, "host_internal.h")).read()
    assert "int " + NAME + "(" in unit and NAME not in pairs
    assert unit.count("pairs_refusals(") == 1 and "hamming_refusals(" not in unit and "family(" not in unit
    entry = unit[unit.index("int " + NAME + "("):]
    assert entry.index("pairs_refusals(") < entry.index("unknown method") < entry.index("hamming_call(") < entry.index("umi_run(")
    for src in (unit, open(os.path.join(CSRC, "collapse_step.h")).read(), open(os.path.join(CSRC, "umi_step.h")).read()):
        assert "getenv" not in src and "asm" not in src
    for kernel in ("umi_insert_kernel", "umi_lookup_kernel", "umi_gather_kernel", "umi_init_kernel", "umi_relax_kernel", "umi_group_kernel",
                   "umi_expand_kernel"):
        assert len(re.findall(r"__global__[^;{]*\b" + kernel + r"\(", unit)) == 1, kernel
    for name in ("collapse_insert(", "collapse_lookup(", "umi_relax(", "cluster_find(", "pairs_scan_u64(", "pairs_resident_link(", "pairs_resident_records(",
                 "pairs_upload_self("):
        assert name in unit, name
    for name in ("int pairs_upload_self(", "int pairs_resident_link(", "int pairs_resident_records(", "int pairs_scan_u64("):
        assert name in internal and name in pairs, name
    # the walks and the scan exist once, in hamming_pairs.hip; the records never leave the device here
    for kernel in ("pairs_survey_kernel", "pairs_fill_kernel", "pairs_cluster_kernel", "pairs_scan_sums_kernel", "pairs_scan_top_kernel", "pairs_scan_rows_kernel"):
        assert kernel + "<" not in unit and kernel + "," not in unit and kernel + "(" not in unit, kernel
    assert "pairs_take_records" not in unit and "sassy_hip_HammingPair*>(malloc" not in unit
    # relaxed, agent scope, every atomic of the unit
    atomics = re.findall(r"__hip_atomic_\w+\([^;]*;", unit)
    assert len(atomics) >= 8
    for call in atomics:
        assert "__ATOMIC_RELAXED" in call and "__HIP_MEMORY_SCOPE_AGENT" in call, call
    # the host loop is bounded
    assert "rounds > n_u" in unit


def test_helper_on_the_hand_written_case():
    for method in uref.METHODS:
        labels, sizes, reps, counts = uref.expected_umi_groups("dna", uref.HAND, uref.HAND_K, method)
        assert all(col.dtype == np.uint32 for col in (labels, sizes, reps, counts))
        assert reps.tolist() == uref.HAND_REPS and counts.tolist() == uref.HAND_COUNTS, method
        assert labels.tolist() == uref.HAND_LABELS[method] and sizes.tolist() == uref.HAND_SIZES[method], method
    # k = 0: nothing is a neighbour, every method is `unique`
    for method in uref.METHODS:
        assert uref.expected_umi_groups("dna", uref.HAND, 0, method)[0].tolist() == uref.HAND_REPS
    # the count rule at its edge: 7 absorbs 4 (7 >= 7), 6 does not; equal counts of 1 point at each other, the smaller index opens
    seven = [b"AAAA"] * 7 + [b"AAAT"] * 4
    assert set(uref.expected_umi_groups("dna", seven, 1)[0].tolist()) == {0}
    assert uref.expected_umi_groups("dna", seven[1:], 1)[0].tolist() == [0] * 6 + [6] * 4
    assert uref.expected_umi_groups("dna", [b"AAAT", b"AAAA"], 1)[0].tolist() == [0, 0]
    assert uref.expected_umi_groups("dna", [b"AAAT", b"AAAA", b"AAAT", b"AAAA"], 1)[0].tolist() == [0, 1, 0, 1]   # (2 < 2 * 2 - 1)
    # a chain of count-1 sequences is one group, as it is one component
    chain = [b"AAAA", b"AAAT", b"AATT", b"ATTT", b"TTTT"]
    assert uref.expected_umi_groups("dna", chain[::-1], 1)[0].tolist() == [0] * 5
    # what folds: case under dna / iupac / ascii_ci, not under ascii; Iupac's N matches A and is no duplicate of it
    assert uref.duplicates("dna", [b"ACGT", b"acgt"])[0].tolist() == [0, 0]
    assert uref.duplicates("iupac", [b"ACGN", b"acgn", b"ACGA"])[0].tolist() == [0, 0, 2]
    assert uref.duplicates("ascii", [b"abc", b"ABC", b"abc"])[0].tolist() == [0, 1, 0]
    assert uref.duplicates("ascii_ci", [b"abc", b"ABC", b"ab@"])[0].tolist() == [0, 0, 2]
    labels, sizes, reps, counts = uref.expected_umi_groups("iupac", [b"ACGN", b"ACGA", b"acgn"], 0, "cluster")
    assert (labels.tolist(), sizes.tolist(), reps.tolist(), counts.tolist()) == ([0, 0, 0], [3, 3, 3], [0, 1, 0], [2, 1, 2])
    # rc: a sequence and its reverse complement are neighbours at k = 0, a palindrome's own record is no edge
    assert uref.expected_umi_groups("dna", [b"AAAC", b"GTTT", b"ACGT"], 0, rc=True)[0].tolist() == [0, 0, 2]


# ---------------------------------------------------------------- CLI
def test_cli_cluster_umi_parser(sassy, capsys, tmp_path):
    from sassy_amd import cli
    import argparse
    a = tmp_path / "a.txt"
    a.write_bytes(b"ACGT\nGGCC\n")
    ap = argparse.ArgumentParser()
    cp = cli.cluster_parser(ap.add_subparsers(dest="cmd"))
    assert cp.parse_args([str(a), "-k", "1"]).umi is None                      # (without --umi: the cluster rows as before)
    for method in ("unique", "cluster", "directional"):
        assert cp.parse_args([str(a), "-k", "1", "--umi", method]).umi == method
    with pytest.raises(SystemExit):
        cp.parse_args([str(a), "-k", "1", "--umi", "adjacency"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        cli.main(["cluster", str(a), "-k", "1", "--umi", "directional", "--edit"])
    assert "does not take --edit" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["cluster", str(a), "-k", "255", "--umi", "unique"])
    assert "0 <= k <= 254" in capsys.readouterr().err


def test_cli_umi_row_writer_on_canned_arrays(sassy):
    from sassy_amd import cli
    seqs = [("r%d" % i, s) for i, s in enumerate(uref.HAND)]
    assert cli.umi_header() == "id\trep_id\tcount\tgroup_id\tgroup_size\n"
    cols = [np.array(v, dtype=np.uint32) for v in (uref.HAND_LABELS["directional"], uref.HAND_SIZES["directional"], uref.HAND_REPS, uref.HAND_COUNTS)]
    rows = cli.umi_rows(seqs, *cols)
    assert rows[:5] == ["r0\tr0\t10\tr0\t14\n", "r1\tr1\t4\tr0\t14\n", "r2\tr2\t3\tr2\t3\n", "r3\tr0\t10\tr0\t14\n", "r4\tr4\t1\tr4\t1\n"]
    assert len(rows) == len(uref.HAND) and cli.umi_rows([], *(c[:0] for c in cols)) == []
    assert cli.cluster_header() == "id\tcluster_id\tcluster_size\n"             # (the plain verb's rows are untouched)

    class Canned:
        def umi_groups(self, a, k, method):
            assert (a, k, method) == ([s for _, s in seqs], 1, "directional")
            return cols

    import argparse
    import io
    out = io.StringIO()
    assert cli.run_cluster(argparse.Namespace(umi="directional", edit=False, k=1), Canned(), seqs, out) == 0
    assert out.getvalue() == cli.umi_header() + "".join(rows)
