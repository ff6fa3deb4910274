"""The shared pass's planner (sassy_amd/csrc/pass_planner.h) on the CPU: tests/c/pass_planner_driver.cc, built with the
host compiler and no HIP, feeds it random begin / finish sequences (2 - 4 searches in flight, tickets that can share and
tickets that cannot, two buffers, every value of shared_pass, any finishing order) and checks that every ticket gets
every half exactly once, that both members of a launch get the same range and fit, that no launch has more than two
members and the older ticket leads, that finish never returns with something of its ticket unlaunched, and that
shared_pass 0 / 2 / 3 give whole launches only; and, for a stream of tickets that all fit (shared_pass 4), that every
begin queues exactly one launch and every ticket with a predecessor and a successor shares both of its halves."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("planner") / "pass_planner_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "c", "pass_planner_driver.cc")])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_begin_finish_sequences(driver, seed):
    r = subprocess.run([driver, str(seed), "5000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
    assert int(fields["sequences"]) == 5000
    assert int(fields["shared"]) > 1000 and int(fields["halves"]) > 1000  # (the sequences reach shared and half launches)


def test_planner_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "pass_planner.h")).read()
    assert "#include <hip" not in src and "hipEvent" not in src and "hipStream" not in src
