"""The LDS layout of the shared pass's fused launches (sassy_amd/csrc/pass_lds.h) on the CPU: tests/c/pass_lds_driver.cc,
built with the host compiler, no HIP and -fsanitize=address,undefined, walks every (members 1 / 2) x (kPlaneRaw,
kPlaneWrite, kPlaneRead) x piece length 7 .. 12 and checks that the DP area, the segment state, every member's queue and
its count are disjoint, 16-byte aligned and inside the bytes per wave (each range is written into a buffer of exactly
that size); that the text-staging launches keep their sizes (11 296 bytes per wave, 45 184 per workgroup with two
members, the queues behind an 8 192-byte tile); and that the plane reader's workgroup, its piece-row table included, is at
most 40 960 bytes: four per CU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pass_lds") / "pass_lds_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "c", "pass_lds_driver.cc")])
    return exe


def test_every_layout(driver):
    r = subprocess.run([driver], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
    assert int(fields["cases"]) == 2 * 3 * 6
    assert int(fields["ranges"]) == 6 * (3 * 4 + 3 * 6)  # (dp, state and per member a queue and a count)


def test_layout_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "pass_lds.h")).read()
    assert "#include <hip" not in src and "__device__" not in src and "__host__" not in src


def test_host_and_kernel_take_the_layout_from_the_header():
    csrc = os.path.join(ROOT, "sassy_amd", "csrc")
    kernel = open(os.path.join(csrc, "scan_kernel.hip")).read()
    host = open(os.path.join(csrc, "scan_driver.hip")).read()
    assert "kTile = pass_lds_queues(G, SRC)" in kernel and "kSegState = pass_lds_state(G, SRC).begin" in kernel
    assert "GP.lds_per_wave = pass_lds_per_wave(2, src, F.fuse_queue_cap)" in host
    assert "GP.lds_per_wave = pass_lds_per_wave(1, src, F.fuse_queue_cap)" in host
