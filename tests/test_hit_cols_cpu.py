"""The hit path's 32-bit relative columns (csrc/hit_cols_step.h) without a device: against the 64-bit forms the kernel had,
under sanitizers; the header free of HIP; the kernel's and the host's use of it.  The kernel itself:
tests/test_gpu_pair_trip.py."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")


def test_relative_columns_equal_the_64_bit_forms_under_sanitizers(tmp_path):
    """tests/c/hit_cols_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined.  Every single bit and every pair of bits of a 64-column mask, rem 0 .. 120, k 0 .. 7, on
    blocks at the buffer's first and last columns (both clamps), lanes below 1 024 blocks (a negative origin), lanes just
    under 2^32 blocks, and the windows around those columns, those that begin before byte 0 included: columns and queue
    entries bit for bit those of piece_end_cols and fuse_emit."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hit_cols_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "hit_cols_driver.cc")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    fields = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}
    assert fields["cols"] >= 10_000_000 and fields["windows"] >= 50_000_000
    # neither clamp, no window from byte 0 and no kind of origin is missing
    assert fields["clamped_lo"] >= 1000 and fields["clamped_hi"] >= 100_000 and fields["from_zero"] >= 1_000_000
    assert fields["negative_base"] >= 10 and fields["high_base"] >= 8


def test_header_is_free_of_hip():
    src = open(os.path.join(CSRC, "hit_cols_step.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src and "asm" not in re.sub(r"//.*", "", src)
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstdint>"]
    assert '"hit_cols_step.h"' in open(os.path.join(ROOT, "sassy_amd", "build.py")).read()


def test_the_grouped_pass_uses_it_and_the_host_states_the_domain():
    unit = open(os.path.join(CSRC, "scan_kernel.hip")).read()
    assert '#include "hit_cols_step.h"' in unit
    kernel = unit[unit.index("void filter_dna_kernel(const ScanParams P)"):]
    grouped = kernel[kernel.index("auto pair_hits = "):kernel.index("auto pair_trip = ")]
    # the pair trip's hit path: relative columns, the slots' constants from registers, no 64-bit form and no launch parameter per slot
    assert grouped.count("hit_end_cols(") == 1 and "piece_end_cols(" not in grouped and "piece_rem" not in grouped and "piece_member" not in grouped
    assert unit.count("hit_window(") == 1
    driver = open(os.path.join(CSRC, "scan_driver.hip")).read()
    assert "if (!hit_cols_fits(bpl)) return fail(" in driver
