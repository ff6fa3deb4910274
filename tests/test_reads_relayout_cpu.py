"""The edit-distance batch calls over a resident read batch (sassy_hip_*_reads of the search_many family, sassy_hip_reads_relayout):
everything that needs no device -- the relayout's block arithmetic (sassy_amd/csrc/relayout_step.h) under sanitizers against the
numpy layout, the symbols, the refusals that come before device work, the switch.  The kernel and the calls:
tests/test_gpu_reads_edit.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import relayout_ref as ref  # noqa: E402

CALL_NAMES = ("sassy_hip_search_many_reads", "sassy_hip_min_costs_reads", "sassy_hip_best_pattern_reads", "sassy_hip_best_matches_reads")
SIBLINGS = ("sassy_hip_search_many", "sassy_hip_min_costs", "sassy_hip_best_pattern", "sassy_hip_best_matches")


@pytest.fixture(scope="module")
def sassy():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("relayout") / "relayout_step_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "relayout_step_driver.cc")])
    return exe


def length_lists():
    return (("forward", ref.LENGTHS), ("reversed", ref.LENGTHS[::-1]), ("more", ref.MORE_LENGTHS))


def test_the_lists_reach_the_residues_the_copy_can_go_wrong_at():
    mod16, mod64 = set(), set()
    for _, lens in length_lists():
        for first, count in ((0, len(lens)), (3, 5)):
            for _, starts, _, _ in ref.geometries(lens[first:first + count]):
                mod16 |= set((starts % 16).tolist())
                mod64 |= set((starts % 64).tolist())
    assert {0, 1, 15} <= mod16 and {0, 63} <= mod64, (sorted(mod16), sorted(mod64))
    # the per-text layout with steps == 0 gives an empty read a slot of no bytes: several reads share a start
    starts, total = ref.pertext_starts(ref.LENGTHS, 0)
    assert starts[0] == starts[1] and starts[11] == starts[12] and starts[13] == total
    # and the destination's last block is shorter than 64 bytes, its last piece shorter than 16
    assert any(t % 64 and t % 16 for _, lens in length_lists() for _, _, t, _ in ref.geometries(lens))


def test_step_arithmetic_under_sanitizers(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok checks="), r.stdout + r.stderr
    assert int(r.stdout.split("=")[1]) == 65 * 65 * 16 + 3 * 243 * 9 + 6 * 8 + 256 * 4 * 5, r.stdout


def test_blocks_equal_the_numpy_layout(driver, tmp_path):
    """rl_block over every block of every case, as the kernel runs it, under -fsanitize=address,undefined: the destination is
    byte for byte the numpy layout; no load leaves the source buffer or misses every read, no store passes `total`."""
    cases = 0
    for order, lens in length_lists():
        seqs = ref.sequences(lens)
        src, src_starts = ref.resident(seqs)
        (tmp_path / "src.bin").write_bytes(src.tobytes())
        for first, count in ((0, len(lens)), (3, 5)):
            part = seqs[first:first + count]
            for name, starts, total, pad in ref.geometries([len(s) for s in part]):
                want = ref.layout(part, starts, total, pad)
                head = "%d %d %d %d %d\n" % (len(lens), first, count, total, pad)
                head += "".join("%d %d\n" % (int(a), n) for a, n in zip(src_starts.tolist(), lens))
                head += "".join("%d\n" % a for a in starts.tolist())
                (tmp_path / "case.txt").write_text(head)
                r = subprocess.run([driver, str(tmp_path / "case.txt"), str(tmp_path / "src.bin"), str(tmp_path / "out.bin")],
                                   capture_output=True, text=True, timeout=300)
                assert r.returncode == 0 and r.stdout.startswith("ok blocks=%d " % ((total + 63) // 64)), (order, name, first, r.stdout + r.stderr)
                got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
                assert got.size == want.size, (order, name, first, got.size, want.size)
                msg = ref.first_difference(got, want, starts, first)
                assert msg is None, (order, name, first, count, msg)
                cases += 1
    assert cases == 3 * 2 * 4


def test_step_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "relayout_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "__builtin_amdgcn" not in src
    unit = open(os.path.join(ROOT, "sassy_amd", "csrc", "reads_relayout.hip")).read()
    assert '#include "relayout_step.h"' in unit and "rl_block(" in unit and "asm" not in re.sub(r"//.*", "", unit)


def test_symbols_are_declared_exported_and_listed(sassy):
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rust[rust.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    L = sassy.lib()
    for name in CALL_NAMES + ("sassy_hip_reads_relayout",):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in sassy.EXPORTED_SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", block), name
    # a handle where the sibling takes texts, text_lens, n_texts
    for name, sib in zip(CALL_NAMES, SIBLINGS):
        assert len(getattr(L, name).argtypes) == len(getattr(L, sib).argtypes) - 2, name
    assert len(L.sassy_hip_reads_relayout.argtypes) == 8
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"reads_relayout.hip"' in build and '"relayout_step.h"' in build
    rows = {r[0]: r for r in sassy.option_table()}
    assert rows["many_batch"][1] == "0" and "at most this many bytes" in rows["many_batch"][2]


def test_refusals_that_need_no_handle(sassy):
    """reads == NULL is SASSY_HIP_EINVAL from every entry point, before any device work (a child that sees no device)."""
    code = r'''
import ctypes as C, sassy_amd
L = sassy_amd.lib()
s = sassy_amd.Searcher("iupac", rc=True)
pp, pl = (C.c_char_p * 1)(b"ACGTACGT"), (C.c_size_t * 1)(8)
out, cost = C.c_void_p(), (C.c_uint8 * 8)()
calls = (("search_many_reads", (C.byref(out),)), ("min_costs_reads", (cost, None)), ("best_pattern_reads", (cost, None, None)),
         ("best_matches_reads", (C.byref(out),)))
for name, tail in calls:
    rc = getattr(L, "sassy_hip_" + name)(s._h, pp, pl, 1, None, 1, 0, *tail)
    assert rc == -1 and b"null" in L.sassy_hip_last_error().lower(), (name, rc, L.sassy_hip_last_error())
starts = (C.c_uint64 * 1)(0)
assert L.sassy_hip_reads_relayout(None, 0, 1, starts, 64, 88, 4096, None) == -1
print("ok")
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
