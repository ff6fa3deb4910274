"""The kept code planes' validity (sassy_amd/csrc/plane_cache.h) on the CPU: tests/c/plane_cache_driver.cc, built with the
host compiler and no HIP, runs the cache next to the shared pass's planner the way c_abi.hip does, over EVERY begin /
finish sequence of a given length at 2, 3 and 4 searches in flight (tickets of one buffer, of a second buffer, and tickets
that cannot take planes; finished oldest or newest first; shared_pass 1, 4, 3 and 0), and checks against a model that
no launch reads a half that was not written under the same key since the open count was last zero, that a reader always
names the writer's launch slot while the host has not seen the writer complete (and that slot is still held), that
dropping to zero open tickets forgets everything, that a foreign-key ticket in the middle of a stream neither reads nor
clobbers, that a search with nothing else in flight (serial begin / finish) never asks for a store, writes or reads, and
that a launch error keeps planes away until every open ticket has left."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("planes") / "plane_cache_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "c", "plane_cache_driver.cc")])
    return exe


@pytest.mark.parametrize("depth,events", [(2, 10), (3, 9), (4, 9)])
def test_every_begin_finish_sequence(driver, depth, events):
    r = subprocess.run([driver, str(depth), str(events)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
    # (the sequences reach readers behind a writer still in flight, foreign tickets among written halves, and drains)
    assert int(fields["sequences"]) > 10000
    assert int(fields["reads"]) > 1000 and int(fields["writes"]) > 1000 and int(fields["waits"]) > 1000
    assert int(fields["foreign_raw"]) > 1000 and int(fields["forgets"]) > 1000
    assert int(fields["lone_raw"]) > 1000  # (a search with nothing else in flight: no store, its own launch -- checked per launch)


def test_cache_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "sassy_amd", "csrc", "plane_cache.h")).read()
    assert "#include <hip" not in src and "hipEvent" not in src and "hipStream" not in src
