"""CPU-only: UMI grouping and deduplication of a resident read batch (sassy_hip_umi_groups_reads, sassy_hip_dedup_reads,
DeviceReads.umi_groups, DeviceReads.dedup, `dedup`) -- what needs no device: the definition's helper on the case written out by
hand and against a brute force in plain Python, the arithmetic of dedup_step.h driven by a stand-alone host program under
AddressSanitizer / UBSan, the step header's and the unit's layout, the symbols, every refusal the C calls can raise without a read
batch, the CLI's parser and row writer."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, ROOT)

NAMES = ("sassy_hip_umi_groups_reads", "sassy_hip_dedup_reads")
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")
SEED = 5  # tests/test_gpu_dedup_reads.py groups the same batch


@pytest.fixture(scope="module")
def sassy():
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


@pytest.fixture(scope="module")
def ddref(sassy):   # (the helper's grouping imports the oracle, which the build makes)
    import dedup_reads_ref
    return dedup_reads_ref


# ---------------------------------------------------------------- the definition
def test_helper_reproduces_the_case_written_out_by_hand(ddref):
    reads = ddref.hand_batch()
    uref = ddref.uref
    assert len(reads) == len(uref.HAND) + 2 and [r for r, s in enumerate(reads) if len(s) < 4] == list(ddref.HAND_NO_WINDOW)
    have, wins = ddref.windows(reads, 4)
    assert wins == uref.HAND and [ddref._moved(j) for j in range(len(uref.HAND))] == have
    for method in uref.METHODS:
        label, size, rep, count, n_unique, n_groups, kept, out = ddref.expected_dedup("dna", reads, 4, uref.HAND_K, method)
        assert label[have].tolist() == [have[j] for j in uref.HAND_LABELS[method]] and size[have].tolist() == uref.HAND_SIZES[method]
        assert rep[have].tolist() == [have[j] for j in uref.HAND_REPS] and count[have].tolist() == uref.HAND_COUNTS
        for r in ddref.HAND_NO_WINDOW:
            assert (label[r], size[r], rep[r], count[r]) == (0xFFFFFFFF, 0, 0xFFFFFFFF, 0)
        assert n_unique == 4 and n_groups == len(set(uref.HAND_LABELS[method])) == len(kept)
        assert out == [(reads[r], None) for r in kept.tolist()]
    assert ddref.expected_dedup("dna", reads, 4)[6].tolist() == ddref.HAND_KEPT["directional"] == [2, 5, 18]
    # qualities change the score: a short read of high qualities beats a long one of low ones
    with_q = [(s, (b"~" if r == 0 else b"!") * len(s)) for r, s in enumerate(reads)]
    assert ddref.expected_dedup("dna", with_q, 4)[6].tolist()[0] == 0
    # from the 3' end, and behind a spacer
    assert ddref.windows([b"AACCGGTT", b"AAC"], 4, at=1, end3=True) == ([0], [b"CGGT"])
    assert ddref.windows([b"AACCGGTT", b"AACCG"], 4, at=1) == ([0, 1], [b"ACCG", b"ACCG"])


def _brute_kept(label, score):
    """the kept read of every group member by member in plain Python: the highest score, then the smallest index"""
    kept = []
    for g in sorted(set(l for l in label if l != 0xFFFFFFFF)):
        members = [r for r, l in enumerate(label) if l == g]
        top = max(score[r] for r in members)
        kept.append(min(r for r in members if score[r] == top))
    return sorted(kept)


def test_helper_against_a_brute_force_on_random_batches(ddref):
    rnd = random.Random(13)
    uref = ddref.uref
    mixed = ties = short = 0
    for _ in range(40):
        profile = rnd.choice(("dna", "iupac"))
        letters = b"ACGT" if profile == "dna" else b"ACGTNacgtRYU"
        m, at, end3 = rnd.choice((1, 3, 6, 9)), rnd.randrange(3), rnd.random() < 0.5
        method, k, rc = rnd.choice(uref.METHODS), rnd.choice((0, 1, 2)), rnd.random() < 0.3
        umis = [bytes(rnd.choice(letters) for _ in range(m)) for _ in range(4)]
        reads = []
        for _ in range(30):
            la = rnd.randrange(at + m + 6)
            seq = bytearray(rnd.choice(letters) for _ in range(la))
            if la >= at + m:
                w = la - at - m if end3 else at
                seq[w:w + m] = rnd.choice(umis)
                if rnd.random() < 0.3:                        # (a neighbour of one of the keys)
                    seq[w + rnd.randrange(m)] = rnd.choice(letters)
            reads.append((bytes(seq), bytes(rnd.choice((40, 41)) for _ in range(la))) if profile == "dna" else bytes(seq))
        label, size, rep, count, n_unique, n_groups, kept, out = ddref.expected_dedup(profile, reads, m, k, method, at, end3, rc)
        seqs, quals = ddref.split(reads)
        have = [r for r, s in enumerate(seqs) if len(s) >= at + m]
        wins = [seqs[r][(len(seqs[r]) - at - m if end3 else at):][:m] for r in have]
        l, z, p, c = uref.expected_umi_groups(profile, wins, k, method, rc=rc)
        for r in range(len(reads)):
            if r in have:
                j = have.index(r)
                assert (label[r], size[r], rep[r], count[r]) == (have[l[j]], z[j], have[p[j]], c[j])
            else:
                assert (label[r], size[r], rep[r], count[r]) == (0xFFFFFFFF, 0, 0xFFFFFFFF, 0)
        score = [sum(q) if q is not None else len(s) for s, q in zip(seqs, quals)]
        assert kept.tolist() == _brute_kept(label.tolist(), score) and len(kept) == n_groups
        assert out == [(seqs[r], quals[r]) for r in kept.tolist()]
        d = ddref.describe(profile, reads, m, k, method, at, end3, rc)
        mixed, ties, short = mixed + d["mixed_groups"], ties + d["score_ties"], short + d["no_window"]
    assert mixed > 20 and ties > 20 and short > 100, (mixed, ties, short)


def test_the_seeded_batch_is_non_trivial(ddref):
    """The batch the GPU tests deduplicate, by the helper alone: groups of more than one distinct key, reads without a window, groups
    whose best score is shared -- and the score decides: qualities keep other reads than lengths do."""
    for n in (257, 1025, 4001):
        d = ddref.describe("dna", ddref.seeded_batch(n, SEED), 12)
        assert d["mixed_groups"] * 4 > d["n_groups"] and d["no_window"] * 12 > n and d["score_ties"] >= 2 and d["multi"] * 2 > d["n_groups"], (n, d)
        assert d["n_unique"] > d["n_groups"] > n // 12
    reads = ddref.seeded_batch(900, SEED, n_umis=50)
    label = ddref.expected_groups("dna", reads, 12)[0]
    a, b = ddref.kept_of(label, ddref.scores(reads)), ddref.kept_of(label, ddref.scores([s for s, _ in reads]))
    assert len(a) == len(b) and (a != b).sum() > 10
    d = ddref.describe("dna", ddref.seeded_batch(500, SEED + 2, rc_mix=True, n_umis=25), 12, rc=True)
    e = ddref.describe("dna", ddref.seeded_batch(500, SEED + 2, rc_mix=True, n_umis=25), 12, rc=False)
    assert d["n_groups"] < e["n_groups"], (d, e)                  # the reverse-complemented keys join their groups under rc only


# ---------------------------------------------------------------- the step header
MS = (1, 8, 31, 32, 33, 63, 64, 65, 96, 127, 128)
ATS = list(range(16)) + [63, 64, 65, 127, 128, 129, 383, 384, 385]


def test_step_arithmetic_against_pairs_encode_under_sanitizers(tmp_path):
    """tests/c/dedup_step_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: dedup_step.h as the kernels call it, a lane simulated, against pairs_encode of the window."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dedup_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "c", "dedup_step_driver.cc")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    fields = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}
    # per profile, key length, place and end: the read lengths at + m - 1, at + m, at + m + 1, 0 and 512
    lens = lambda at, m: [la for la in (at + m - 1, at + m, at + m + 1, 0, 512) if la <= 512]
    per = sum(len(lens(at, m)) for m in MS for at in ATS if at + m <= 512)
    windows = sum(sum(1 for la in lens(at, m) if la >= at + m) for m in MS for at in ATS if at + m <= 512)
    assert fields["cases"] == 2 * 2 * per and fields["windows"] == 2 * 2 * windows and fields["no_window"] == fields["cases"] - fields["windows"], fields
    assert fields["strands"] == 2 * fields["windows"] and fields["windows"] > 3000, fields
    assert fields["refusals"] == 21 and fields["reductions"] == 2000 and fields["sums"] == 17, fields


def test_step_header_is_free_of_hip_and_the_driver_stands_alone():
    src = open(os.path.join(CSRC, "dedup_step.h")).read()
    code = re.sub(r"//.*", "", src)
    assert "#include <hip" not in src and "hipStream" not in src and "getenv" not in src
    assert "__builtin_amdgcn" not in src and "__HIP_DEVICE_COMPILE__" not in src and "asm" not in code and "switch" not in code
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>", '#include "demux_step.h"']
    for fn in ("ddp_refusal", "ddp_reverse_rows", "ddp_pack_block", "ddp_window_planes", "ddp_piece_sum", "ddp_key", "ddp_key_read"):
        assert re.search(r"\b" + fn + r"\s*\(", src), fn
    # the window, the relation and the complement are not restated: they are the siblings'
    assert "trm_window_block(" in code and "pairs_row_code(" in code and "ovl_complement(" in code and "pairs_row_mask(" in code
    assert "ham_iupac_nib" not in code and ">> 1) & 3" not in code and "'A'" not in code and "la - at" not in code
    driver = open(os.path.join(ROOT, "tests", "c", "dedup_step_driver.cc")).read()
    assert "int main(" in driver and "#include <hip" not in driver and "__global__" not in driver and "dedup_step.h" in driver
    assert "pairs_encode(" in driver and "pairs_reverse_complement(" in driver


def test_source_layout():
    """The entry points live in dedup_reads.hip with six kernels, no inline assembly and no environment; the grouping behind the
    upload, the scan, the layout scan and the write kernel are the siblings', with one definition each; umi_groups.hip and the
    pair unit kept their kernels."""
    unit = open(os.path.join(CSRC, "dedup_reads.hip")).read()
    code = re.sub(r"//.*", "", unit)
    for name in NAMES:
        assert "int " + name + "(" in unit
    assert "asm" not in code and "getenv" not in code and "switch" not in code and "sw." not in code
    for kernel in ("dedup_flag_kernel", "dedup_encode_kernel", "dedup_scatter_kernel", "dedup_score_kernel", "dedup_keep_kernel", "dedup_compact_kernel"):
        assert len(re.findall(r"__global__[^;{]*\b" + kernel + r"\(", unit)) == 1, kernel
    assert code.count("__global__") == 6
    assert code.count("__hip_atomic_fetch_max(") == 1 and "__HIP_MEMORY_SCOPE_AGENT" in code and code.count("atomic") == 1
    for call in ("ddp_refusal(", "ddp_window_planes<P, RC>(", "dmx_window(", "dmx_has_window(", "umi_groups_resident(", "pairs_scan_u64(", "reads_require_plain(",
                 "reads_layout_windows(", "write_windows(", "reads_empty_buffers(", "reads_new_batch("):
        assert call in code, call
    shared = open(os.path.join(CSRC, "reads_call.hip")).read()
    assert len(re.findall(r"\nint reads_require_plain\(", shared)) == 1 and shared.count("reads_plain(") == 1   # the Dna look: one owner, called here
    frame = open(os.path.join(CSRC, "host_internal.h")).read()
    frame = frame[frame.index("\nint reads_new_batch("):]
    assert frame[:frame.index("\n}\n")].count("hamming_call(") == 1 and frame.count("\nint reads_new_batch(") == 1   # the frame: one owner, called here
    assert "fastq_rec_" not in code and "reads_window_write_kernel<" not in code and "pairs_upload" not in code and "uint4" in code
    host = open(os.path.join(CSRC, "host_internal.h")).read()
    assert "int umi_groups_resident(" in host and "DevBuf<uint8_t> d_dedup;" in host and "int pairs_upload_self(" in host
    umi = open(os.path.join(CSRC, "umi_groups.hip")).read()
    assert len(re.findall(r"\nint umi_groups_resident\(", umi)) == 1 and len(re.findall(r"\nint umi_run\(", umi)) == 1
    assert umi.count("pairs_upload_self(") == 1 and umi.index("pairs_upload_self(s, a") > umi.index("\nint umi_groups_resident(")
    assert re.sub(r"//.*", "", umi).count("__global__") == 7     # insert, lookup, gather, init, relax, group, expand: as before
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"dedup_reads.hip"' in build and '"dedup_step.h"' in build


# ---------------------------------------------------------------- the surface
def test_symbols_are_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    L = sassy.lib()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
    assert re.search(r"#define SASSY_HIP_DEDUP_END3\s+1u\b", hdr) and sassy.DEDUP_END3 == 1 and "DEDUP_END3: u32 = 1" in rust
    assert len(L.sassy_hip_umi_groups_reads.argtypes) == 13 and len(L.sassy_hip_dedup_reads.argtypes) == 15
    for attr in ("umi_groups", "dedup"):
        assert hasattr(sassy.DeviceReads, attr), attr
    assert callable(sassy.dedup_reads) and hasattr(sassy.Deduped, "free")
    doc = hdr[hdr.index("/* UMI grouping and deduplication of a resident read batch"):hdr.index("int " + NAMES[0])]
    for word in ("score << 32 | (0xFFFFFFFF - r)", "text_bytes == 64", "sassy_hip_reads_free", "1 <= m <= 128", "at + m <= 512", "UINT32_MAX",
                 "SASSY_HIP_DEDUP_END3", "filtered = 12", "6 for the groups call", "16 for the dedup call", "scan_launches = 0", "no kernel launched",
                 "tests/helpers/dedup_reads_ref.py", "k >= m is cut to m"):
        assert word in doc, word
    import inspect
    sig = inspect.signature(sassy.DeviceReads.umi_groups).parameters
    assert [(k, v.default) for k, v in list(sig.items())[3:]] == [("k", 1), ("method", "directional"), ("at", 0), ("end3", False)]
    sig = inspect.signature(sassy.DeviceReads.dedup).parameters
    assert list(sig)[:3] == ["self", "searcher", "umi_len"]
    assert [(k, v.default) for k, v in list(sig.items())[3:]] == [("k", 1), ("method", "directional"), ("at", 0), ("end3", False), ("with_columns", False)]
    assert list(inspect.signature(sassy.dedup_reads).parameters)[:3] == ["searcher", "reads", "umi_len"]


def test_searcher_gained_no_public_method(sassy):
    """The new surface is DeviceReads' and the module's: Searcher and its base classes have the public methods they had."""
    import inspect
    exempt = ("set_", "with_", "get_", "enable_", "_")
    inherited = [name for base in sassy.Searcher.__mro__[1:] if base is not object
                 for name, f in vars(base).items() if inspect.isfunction(f) and not name.startswith(exempt)]
    assert inherited == ["trim_reads"], inherited
    own = [name for name, f in vars(sassy.Searcher).items() if inspect.isfunction(f) and not name.startswith(exempt)]
    assert len(own) == 38, len(own)
    assert not any("dedup" in name or "groups_reads" in name for name in dir(sassy.Searcher))


def test_refusals_come_before_any_device_work(sassy):
    """Every refusal the C calls can raise without a read batch, with its code and a message that names the reason, in their
    order, in a child that sees no device; then the loud failure where there is none.  The refusals that read the batch are the
    same function's next lines: the driver above walks them, the GPU tests raise them."""
    code = r'''
import ctypes as C, sassy_amd
L = sassy_amd.lib()
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -3
FAKE = 0x7000000   # a batch pointer that is never read: every refusal below comes before the batch is looked at
def call(which, s, reads=FAKE, at=0, m=12, k=1, method=2, flags=0, s_null=False, out=True):
    label = (C.c_uint32 * 4)()
    sz = C.c_size_t(0)
    h = None if s_null else s._h
    if which == "groups":
        rc = L.sassy_hip_umi_groups_reads(h, reads, at, m, k, method, flags, label if out else None, None, None, None, C.byref(sz), None)
        return rc, L.sassy_hip_last_error().decode(), None
    handle = C.c_void_p(7)
    rc = L.sassy_hip_dedup_reads(h, reads, at, m, k, method, flags, None, None, None, None, None, None, C.byref(sz), C.byref(handle) if out else None)
    return rc, L.sassy_hip_last_error().decode(), handle.value if out else None
def refused(s, want, word, **kw):
    for which, who in (("groups", "umi_groups_reads"), ("dedup", "dedup_reads")):
        rc, msg, handle = call(which, s, **kw)
        assert rc == want and word.replace("WHO", who) in msg and "no usable HIP device" not in msg and handle is None, (which, rc, msg, want, word, handle)
dna, iupac = sassy_amd.Searcher("dna", rc=False), sassy_amd.Searcher("iupac", rc=True)
ascii_ = sassy_amd.Searcher("ascii", rc=False)
everything = dict(flags=2, method=3, m=0, at=600, reads=None, out=False)   # each refusal hides the ones behind it
refused(ascii_, EINVAL, "WHO() must not be null", s_null=True, **everything)
refused(ascii_, EINVAL, "WHO takes SASSY_HIP_DEDUP_END3 only", **everything)
for flags in (2 | 1, 2, 1 << 20, sassy_amd.KEEP_QUALITY << 8 | 1):
    refused(dna, EINVAL, "WHO takes SASSY_HIP_DEDUP_END3 only", flags=flags)
everything.pop("flags")
refused(ascii_, EINVAL, "WHO: unknown method 3 (0 unique, 1 cluster, 2 directional)", **everything)
everything.pop("method")
refused(ascii_, EINVAL, "WHO: m must be 1 .. 128 (got 0)", **everything)
everything["m"] = 129
refused(ascii_, EINVAL, "WHO: m must be 1 .. 128 (got 129)", **everything)
everything["m"] = 12
refused(ascii_, EINVAL, "WHO: at + m = 612 reaches past", **everything)
refused(ascii_, EINVAL, "WHO: at + m = 513 reaches past", at=385, m=128, reads=None, out=False)
for alphabet in ("ascii", "ascii_ci"):
    refused(sassy_amd.Searcher(alphabet, rc=False), EINVAL, "use a dna or an iupac searcher", at=384, m=128, reads=None, out=False)
refused(sassy_amd.Searcher("iupac", rc=False, alpha=0.5), EUNSUPPORTED, "overhang", reads=None, out=False)
refused(sassy_amd.Searcher("dna", rc=False).only_best_match(), EUNSUPPORTED, "only_best_match", reads=None, out=False)
refused(sassy_amd.Searcher("dna", rc=False).with_max_n_frac(0.2), EUNSUPPORTED, "WHO does not take max_n_frac", reads=None, out=False)
refused(dna, EINVAL, "WHO() must not be null", reads=None, out=False)
refused(iupac, EINVAL, "WHO() must not be null", reads=None, flags=1, k=1 << 40, method=0, m=128, at=384)
# the Python calls: lists go through from_sequences, which refuses before anything else and then needs the device -- loudly
for args, word in ((([(b"AC\nGT", b"IIIII")], 4), "sequence 0 holds a line end"), (([(b"ACGT", b"III")], 4), "quality 0 has 3 bytes, its sequence 4"),
                   (([b"ACGT"], 4), "no usable HIP device"), (([], 4), "no usable HIP device")):
    try:
        sassy_amd.dedup_reads(dna, *args)
    except sassy_amd.SassyHipError as e:
        assert word in str(e), (word, e)
    else:
        raise SystemExit(3)
class Stub(sassy_amd.DeviceReads):
    def __init__(self):
        self._h = None
for fn, word in ((lambda: Stub().dedup(dna, 4), "freed"), (lambda: Stub().umi_groups(dna, 4), "freed")):
    try:
        fn()
    except sassy_amd.SassyHipError as e:
        assert word in str(e), (word, e)
    else:
        raise SystemExit(4)
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_python_argument_checks(sassy):
    class Stub(sassy.DeviceReads):
        def __init__(self):
            self._h = 1

        def __len__(self):
            return 0

        def free(self):
            self._h = None

    for kw, word in ((dict(method="adjacency"), "method must be one of unique, cluster, directional"), (dict(k=-1), "negative"), (dict(at=-1), "negative"),
                     (dict(at=1 << 32), "32 bits")):
        for call in (Stub().dedup, Stub().umi_groups):
            with pytest.raises(sassy.SassyHipError, match=word):
                call(None, 12, **kw)


# ---------------------------------------------------------------- CLI
def test_cli_dedup_parser_and_rows(sassy, capsys, tmp_path):
    from sassy_amd import cli
    import argparse
    ap = argparse.ArgumentParser()
    dp = cli.dedup_parser(ap.add_subparsers(dest="cmd"))
    args = dp.parse_args(["in.fq", "--umi-len", "12", "-o", "out.fq"])
    assert (args.input, args.umi_len, args.at, args.end3, args.k, args.method, args.alphabet, args.output, args.mate, args.mate_out, args.tsv) == \
        ("in.fq", 12, 0, False, 1, "directional", "dna", "out.fq", "", "", "")
    args = dp.parse_args(["in.fq", "--umi-len", "8", "--at", "3", "--end3", "-k", "2", "--method", "cluster", "--alphabet", "IUPAC", "-o", "o.fq",
                          "--mate", "r2.fq", "--mate-out", "o2.fq", "--tsv", "rows.tsv"])
    assert (args.umi_len, args.at, args.end3, args.k, args.method, args.alphabet, args.mate, args.mate_out, args.tsv) == \
        (8, 3, True, 2, "cluster", "iupac", "r2.fq", "o2.fq", "rows.tsv")
    for argv in (["in.fq", "-o", "out.fq"], ["in.fq", "--umi-len", "12"], ["--umi-len", "12", "-o", "out.fq"],
                 ["in.fq", "--umi-len", "12", "-o", "out.fq", "--method", "adjacency"], ["in.fq", "--umi-len", "12", "-o", "out.fq", "--alphabet", "ascii"]):
        with pytest.raises(SystemExit):
            dp.parse_args(argv)
    capsys.readouterr()
    out = str(tmp_path / "out.fq")
    base = ["dedup", "in.fq", "-o", out]
    for argv in (["--umi-len", "0"], ["--umi-len", "129"], ["--umi-len", "12", "--at", "-1"], ["--umi-len", "12", "-k", "-1"]):
        with pytest.raises(SystemExit):
            cli.main(base + argv)
        assert "dedup takes 1 <= --umi-len <= 128" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(base + ["--umi-len", "128", "--at", "385"])
    assert "reach past 512" in capsys.readouterr().err
    for argv in (["--mate", "r2.fq"], ["--mate-out", "o2.fq"]):
        with pytest.raises(SystemExit):
            cli.main(base + ["--umi-len", "12"] + argv)
        assert "given together" in capsys.readouterr().err
    assert not os.path.exists(out)   # nothing above got as far as the device or the files
    label = np.array([0, 0, 0xFFFFFFFF, 3], dtype=np.uint32)
    rows = cli.dedup_rows(["r0 x", "r1", "r2", "r3"], label, np.array([2, 2, 0, 1]), np.array([1, 1, 0, 1]), np.array([1, 3], dtype=np.uint64))
    assert rows == ["r0 x\tr0 x\t2\t1\t0\n", "r1\tr0 x\t2\t1\t1\n", "r2\t-\t0\t0\t0\n", "r3\tr3\t1\t1\t1\n"]
    assert cli.DEDUP_HEADER == "read_id\tlabel_id\tsize\tcount\tkept\n"
