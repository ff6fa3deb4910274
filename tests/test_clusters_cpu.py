"""CPU-only: the surface of the clustering calls (sassy_hip_hamming_clusters, sassy_hip_edit_clusters, the Python methods,
the `cluster` verb) -- what needs no device: the symbols, every refusal with its code and message before any device work,
the loud failure without a device, the union step of cluster_step.h driven by a stand-alone host program under
AddressSanitizer / UBSan and under ThreadSanitizer, the source layout the pair calls' tests pin, the helper on a hand-written
case, the CLI's parser and row writer."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import clusters_ref as cref  # noqa: E402

NAMES = ("sassy_hip_hamming_clusters", "sassy_hip_edit_clusters")
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


@pytest.fixture(scope="module")
def sassy():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


def test_symbols_are_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    L = sassy.lib()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
        assert re.search(r"pub fn\s+" + name[len("sassy_hip_"):] + r"\s*\(", rust), name
        assert getattr(L, name).restype is not None and len(getattr(L, name).argtypes) == 9
    assert hasattr(sassy.Searcher, "hamming_clusters") and hasattr(sassy.Searcher, "edit_clusters")
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"clusters.hip"' in build and '"cluster_step.h"' in build
    # the stats' codes are documented where the others are
    assert re.search(r"\b10: the link walk of sassy_hip_hamming_clusters", hdr) and re.search(r"\b11: the link walk of sassy_hip_edit_clusters", hdr)


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal of both entry points with its code and a message that names the reason, in a child that sees no device:
    a call that got as far as the device would say 'no usable HIP device' instead.  Then valid arguments: that message."""
    code = r'''
import ctypes as C, numpy as np, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
A = b"ACGTACGT" + b"TTTTACGT"
def call(which, s, a=A, n=2, m=8, k=1, flags=0, out=True, s_null=False, sizes=True, count=True):
    h = None if s_null else s._h
    label = np.zeros(16, dtype=np.uint32)
    size = np.zeros(16, dtype=np.uint32)
    nc = C.c_size_t()
    f = L.sassy_hip_hamming_clusters if which == "hamming" else L.sassy_hip_edit_clusters
    rc = f(h, a, n, m, k, flags, label.ctypes.data if out else None, size.ctypes.data if sizes else None, C.byref(nc) if count else None)
    return rc, L.sassy_hip_last_error().decode()
def refused(which, s, want, word, **kw):
    rc, msg = call(which, s, **kw)
    assert rc == want and word in msg and "no usable HIP device" not in msg, (which, rc, msg, want, word)
dna = sassy_amd.Searcher("dna", rc=False)
for which, limit in (("hamming", 128), ("edit", 64)):
    name = which + "_clusters"
    # the family's own checks
    refused(which, sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang")
    refused(which, sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match")
    refused(which, sassy_amd.Searcher("ascii", rc=True), EUNSUPPORTED, "reverse complement is not defined")
    refused(which, sassy_amd.Searcher("ascii_ci", rc=True), EUNSUPPORTED, "reverse complement is not defined")
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, "not valid IUPAC", a=b"ACGTACGT" + b"ACQTACGT")
    refused(which, sassy_amd.Searcher("iupac", rc=True), EINVAL, name + ": list a)", a=b"ACGTACGT" + b"ACQTACGT")
    if which == "hamming":  # (65 distinct bytes need m >= 65)
        for alphabet in ("ascii", "ascii_ci"):
            refused(which, sassy_amd.Searcher(alphabet, rc=False), EUNSUPPORTED, "distinct bytes (pattern 1 has 65)", a=b"x" * 65 + bytes(range(128, 193)), m=65)
    # there is no text span for max_n_frac
    refused(which, sassy_amd.Searcher("dna", rc=False).with_max_n_frac(0.2), EUNSUPPORTED, name + " does not take max_n_frac")
    # the shape
    refused(which, dna, EINVAL, "must be at least 1", m=0)
    refused(which, dna, EINVAL, "must be <= %d" % limit, a=b"A" * (2 * limit + 2), m=limit + 1)
    refused(which, dna, EINVAL, "k must be <= 254", k=255)
    refused(which, dna, EINVAL, "k must be <= 254", k=0x80000000)
    refused(which, dna, EINVAL, name + " needs at least one sequence", n=0)
    for flags in (sassy_amd.WITHOUT_TRACE, sassy_amd.ALL_MINIMA, sassy_amd.TEXT_ON_DEVICE, sassy_amd.TEXT_UNCHANGED, sassy_amd.LINE_SPANS, 1 << 20):
        refused(which, dna, EINVAL, name + " takes no flags", flags=flags)
    refused(which, dna, EUNSUPPORTED, "2^31 - 1", n=1 << 31)
    refused(which, dna, EINVAL, name + "() must not be null", out=False)
    refused(which, dna, EINVAL, "must not be null", a=None)
    refused(which, dna, EINVAL, "must not be null", s_null=True)
    # valid arguments get as far as the device: every alphabet, the limits themselves, the optional outputs left out
    for s, kw in ((dna, {}), (dna, dict(sizes=False, count=False)), (sassy_amd.Searcher("dna", rc=True), dict(k=254)),
                  (sassy_amd.Searcher("iupac", rc=True), dict(a=b"ACGTNNRY" * 2)), (sassy_amd.Searcher("ascii", rc=False), {}),
                  (sassy_amd.Searcher("ascii_ci", rc=False), dict(a=b"x" * (2 * limit), m=limit)), (dna, dict(a=b"AC", m=1)), (dna, dict(n=1))):
        rc, msg = call(which, s, **kw)
        assert rc == ENODEVICE and "no usable HIP device" in msg, (which, rc, msg)
# the Python methods: refusals of their own, then the same loud failure
for method in ("hamming_clusters", "edit_clusters"):
    f = getattr(dna, method)
    for args, word in ((([b"ACGT", b"ACG"],), "sequence 1 has 3 bytes"), (([b"ACGT", sassy_amd.parse_classes(b"a[bc]")],), "ClassPattern"),
                       ((np.zeros((2, 4), dtype=np.int32),), "uint8 array"), ((np.zeros((4, 4), dtype=np.uint8)[:, ::2],), "C-contiguous"),
                       (([b"ACGT"], 300), "k must be <= 254"), (([],), method + " needs at least one sequence"),
                       ((np.zeros((0, 4), dtype=np.uint8),), "needs at least one sequence"), (([b"ACGT", b"AAAA"],), "no usable HIP device"),
                       ((np.frombuffer(b"ACGTAAAA", dtype=np.uint8).reshape(2, 4), 1), "no usable HIP device")):
        try:
            f(*args)
        except sassy_amd.SassyHipError as e:
            assert word in str(e), (method, word, e)
        else:
            raise SystemExit(3)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def _driver(tmp_path, name, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all",
                           "-pthread", "-o", exe, os.path.join(ROOT, "tests", "c", "cluster_step_driver.cc")])
    return exe


def _run_driver(exe, seeds):
    for seed in seeds:
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
        assert int(fields["graphs"]) == 5 * 8 and int(fields["threaded"]) == 5 * 8 and int(fields["links"]) > 10000


def test_union_step_against_a_sequential_union_find_under_sanitizers(tmp_path):
    """tests/c/cluster_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: cluster_step.h with std::atomic on paths, stars, cliques, forests and mixtures of up to
    4000 nodes -- parent[x] <= x and no value rising after every link, root = component minimum at the end, and the same
    labels when up to 8 threads link the edges in another order."""
    _run_driver(_driver(tmp_path, "cluster_step_driver", "address,undefined"), ("1", "2", "3"))


def test_union_step_from_threads_under_thread_sanitizer(tmp_path):
    """The same program built with -fsanitize=thread: every access to the forest is an atomic one."""
    _run_driver(_driver(tmp_path, "cluster_step_driver_tsan", "thread"), ("4", "5"))


def test_driver_is_a_stand_alone_program():
    text = open(os.path.join(ROOT, "tests", "c", "cluster_step_driver.cc")).read()
    assert "int main(" in text and "#include <hip" not in text and "__global__" not in text
    assert "cluster_step.h" in text and "std::atomic" in text and "std::thread" in text


def test_step_header_stays_free_of_hip_and_states_its_rules():
    src = open(os.path.join(CSRC, "cluster_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "getenv" not in src
    assert "__builtin_amdgcn" not in src and "__HIP_DEVICE_COMPILE__" not in src and "asm" not in src
    for name in ("cluster_find", "cluster_link", "cluster_lower", "cluster_join"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    for rule in ("parent[x] <= x", "LOWERS", "ROOTS only", "lock-free", "No thread ever waits"):
        assert rule in src, rule
    # no plain store and no wait in it: the policy's two operations are all that touches the forest (the comments name the
    # device's atomics, the code does not)
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "__hip_atomic" not in code and "parent" not in code
    assert set(re.findall(r"\bmem\.(\w+)\(", code)) == {"load", "cas"}
    # the kernels and the flatten pass share it; the device policy is HIP's atomics at agent scope
    for unit, names in (("hamming_pairs.hip", ("pairs_cluster_kernel", "cluster_join(")), ("edit_pairs.hip", ("edit_cluster_kernel", "cluster_join(")),
                        ("clusters.hip", ("cluster_init_kernel", "cluster_flatten_kernel", "cluster_find("))):
        text = open(os.path.join(CSRC, unit)).read()
        for name in names:
            assert name in text, (unit, name)
    policy = open(os.path.join(CSRC, "host_internal.h")).read()
    policy = policy[policy.index("struct ClusterDeviceMem"):]
    policy = policy[:policy.index("\n};\n")]
    assert "__hip_atomic_load" in policy and "__hip_atomic_compare_exchange_strong" in policy and policy.count("__HIP_MEMORY_SCOPE_AGENT") == 2


def test_source_layout_the_pair_tests_pin():
    """The entry points live in clusters.hip and reach the pair units through one launcher each; the refusals are the pair
    calls' functions, still defined once where they were and still called from nowhere else in those units."""
    pairs = open(os.path.join(CSRC, "hamming_pairs.hip")).read()
    edit = open(os.path.join(CSRC, "edit_pairs.hip")).read()
    unit = open(os.path.join(CSRC, "clusters.hip")).read()
    internal = open(os.path.join(CSRC, "host_internal.h")).read()
    assert pairs.count("hamming_refusals(") == 1 and pairs.count("pairs_refusals(") == 3 and pairs.count("family(") == 2
    assert edit.count("hamming_refusals(") == 1 and edit.count("edit_refusals(") == 3 and edit.count("family(") == 2
    assert "asm" not in edit and "asm" not in open(os.path.join(CSRC, "edit_pairs_step.h")).read()
    for src in (pairs, edit, unit):
        assert "getenv" not in src and "asm volatile" not in src and "__asm" not in src
    assert "sassy_hip_hamming_clusters" not in pairs and "sassy_hip_edit_clusters" not in edit
    for name in ("int pairs_refusals(", "int edit_refusals(", "int pairs_link_components(", "int edit_link_components("):
        assert name in internal, name
    for src, launcher, counted in ((pairs, "int pairs_link_components(", ("pairs_refusals(", "hamming_refusals(", "family(")),
                                   (edit, "int edit_link_components(", ("edit_refusals(", "hamming_refusals(", "family("))):
        body = src[src.index(launcher):]
        body = body[:body.index("\n}\n")]
        for word in counted:
            assert word not in body, (launcher, word)
        assert "kPairsSelfPairs" in body and "kWalkCluster" in body
    # clusters.hip: refusals before the device, no copy of them, no cell matrix
    assert unit.count("pairs_refusals(") == 1 and unit.count("edit_refusals(") == 1 and "hamming_refusals(" not in unit
    call = unit[unit.index("int clusters_call("):]
    assert call.index("pairs_refusals(") < call.index("hamming_call(") < call.index("pairs_link_components(")
    assert "d_pairs_cells" not in unit and "pairs_place_rows" not in unit
    for entry in NAMES:
        assert "int " + entry + "(" in unit
    # the scan's constants and the pass kernels stay where the other tests read them
    assert "constexpr uint32_t kScanItems = 8, kScanBlock = 256 * kScanItems;" in pairs
    for kernel in ("pairs_nearest_kernel", "pairs_rows_kernel", "pairs_scan_sums_kernel", "pairs_scan_top_kernel", "pairs_scan_rows_kernel"):
        assert len(re.findall(r"__global__[^;{]*\b" + kernel + r"\(", pairs)) == 1, kernel
        for src in (edit, unit):
            assert kernel + "(" not in src and kernel + "," not in src, kernel


def test_helper_on_a_hand_written_case():
    for rc, (labels, sizes) in ((False, cref.HAND_FWD), (True, cref.HAND_RC)):
        got_labels, got_sizes = cref.expected_clusters("dna", cref.HAND, cref.HAND_K, rc=rc)
        assert got_labels.dtype == np.uint32 and got_sizes.dtype == np.uint32
        assert got_labels.tolist() == labels and got_sizes.tolist() == sizes, rc
    # k = 0: everything alone; under the edit distance the chain is the same (equal lengths, k = 1)
    assert cref.expected_clusters("dna", cref.HAND, 0)[0].tolist() == [0, 1, 2, 3, 4]
    assert cref.expected_clusters("dna", cref.HAND, 1, edit=True)[0].tolist() == cref.HAND_FWD[0]
    # a shift is two edits and four mismatches
    assert cref.expected_clusters("dna", [b"ACGT", b"CGTA"], 2, edit=True)[0].tolist() == [0, 0]
    assert cref.expected_clusters("dna", [b"ACGT", b"CGTA"], 2)[0].tolist() == [0, 1]
    # Iupac's N joins what it meets: components all the same
    assert cref.expected_clusters("iupac", [b"AAAA", b"CCCC", b"NNNN"], 0)[0].tolist() == [0, 0, 0]
    labels, sizes = cref.components(6, [(5, 4), (4, 3), (1, 2)])
    assert labels.tolist() == [0, 1, 1, 3, 3, 3] and sizes.tolist() == [1, 2, 2, 3, 3, 3]
    # the loop-free union the large GPU case uses gives the same labels: a long path, random sparse edges, no edge at all
    rng = np.random.default_rng(5)
    order = rng.permutation(300)
    for n, i, j in ((300, order[:-1], order[1:]), (2000, rng.integers(0, 2000, 1500), rng.integers(0, 2000, 1500)), (7, [], [])):
        assert cref.components_fast(n, i, j).tolist() == cref.components(n, zip(i, j))[0].tolist()


# ---------------------------------------------------------------- CLI
def test_cli_cluster_parser(sassy, capsys, tmp_path):
    from sassy_amd import cli
    a = tmp_path / "a.txt"
    a.write_bytes(b"ACGT\nGGCC\n")
    with pytest.raises(SystemExit):
        cli.main(["cluster", str(a)])  # no k
    with pytest.raises(SystemExit):
        cli.main(["cluster", str(a), "-k", "255"])
    assert "0 <= k <= 254" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["cluster", str(a), "-k", "1", "--rc", "-a", "ascii"])
    assert "no reverse complement" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["cluster", str(a), "-k", "1", "-a", "protein"])
    ragged = tmp_path / "ragged.txt"
    ragged.write_bytes(b"ACGT\nGGC\n")
    with pytest.raises(SystemExit):
        cli.main(["cluster", str(ragged), "-k", "1"])  # (refused by the front end: no device is asked for)
    assert "sequence 1 has 3 bytes" in capsys.readouterr().err
    empty = tmp_path / "empty.txt"
    empty.write_bytes(b"")
    with pytest.raises(SystemExit):
        cli.main(["cluster", str(empty), "-k", "1"])
    assert "holds no sequence" in capsys.readouterr().err
    import argparse
    ap = argparse.ArgumentParser()
    cp = cli.cluster_parser(ap.add_subparsers(dest="cmd"))
    args = cp.parse_args([str(a), "-k", "2", "--rc", "--edit", "-a", "IUPAC"])
    assert (args.a, args.k, args.rc, args.edit, args.alphabet) == (str(a), 2, True, True, "iupac")
    args = cp.parse_args([str(a), "-k", "0"])
    assert (args.rc, args.edit, args.alphabet) == (False, False, "dna")


def test_cli_cluster_row_writer_on_canned_arrays(sassy):
    from sassy_amd import cli
    seqs = [("u1", b"ACGT"), ("u2", b"ACGA"), ("u3", b"ACCA"), ("u4", b"TTTT"), ("u5", b"AAAT")]
    assert cli.cluster_header() == "id\tcluster_id\tcluster_size\n"
    labels, sizes = (np.array(v, dtype=np.uint32) for v in cref.HAND_RC)
    assert cli.cluster_rows(seqs, labels, sizes) == ["u1\tu1\t3\n", "u2\tu1\t3\n", "u3\tu1\t3\n", "u4\tu4\t2\n", "u5\tu4\t2\n"]
    assert cli.cluster_rows([], labels[:0], sizes[:0]) == []
