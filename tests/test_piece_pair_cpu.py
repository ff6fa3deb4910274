"""The block-pair piece test of the grouped pass (csrc/piece_pair_step.h) without a device: the step against a per-column
comparison of 2-bit codes and against the single-block form, under sanitizers; the header free of HIP; the kernel's use of
it.  The kernel itself: tests/test_gpu_piece_pair.py."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


def test_pair_step_against_the_columns_under_sanitizers(tmp_path):
    """tests/c/piece_pair_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined.  Q = 7 .. 12, eight random slots: an occurrence planted at every end column 0 .. 127 of
    every slot into random planes -- those that reach back into the previous block and from b into a are counted apart --
    and random planes without plants; the masks of a and b against the definition column by column and against two calls
    of the single-block form, and the handed-on halves are b's."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "piece_pair_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "piece_pair_driver.cc")])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}
        # 2 rounds x Q = 7 .. 12 x 8 slots x 128 columns; per round and slot Q - 1 columns reach back: sum = 51
        assert fields["plants"] == 2 * 6 * 8 * 128 and fields["reach_prev"] == fields["reach_a"] == 2 * 8 * 51
        assert fields["random"] == 2 * 6 * 600 and fields["occurrences"] >= fields["plants"] + fields["chance"] and fields["chance"] >= 500


def test_step_header_is_free_of_hip():
    src = open(os.path.join(CSRC, "piece_pair_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "asm" not in re.sub(r"//.*", "", src)
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>"]
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"piece_pair_step.h"' in build


def test_the_grouped_pass_has_one_form():
    """filter_dna_kernel: G = 2 goes through the pair step, once; the loop with scalar constants is in G = 1's branch."""
    unit = open(os.path.join(CSRC, "scan_kernel.hip")).read()
    assert '#include "piece_pair_step.h"' in unit
    kernel = unit[unit.index("void filter_dna_kernel(const ScanParams P)"):]
    assert kernel.count("piece_pair_step<Q, NP>(") == 1 and kernel.count("piece_row_table_fill<Q, NP>(") == 1
    pair, scalar = kernel.index("piece_pair_step<Q, NP>("), kernel.index("__builtin_amdgcn_sbfe((int)b0[pp], j, 1)")
    between = kernel[pair:scalar]
    assert pair < scalar and "} else {\n    if constexpr (SRC == kPlaneRead) {" in between
