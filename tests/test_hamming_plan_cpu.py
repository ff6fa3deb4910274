"""CPU: csrc/hamming_plan.h -- what the host decides for the Hamming family between its launches -- driven without a device."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_header_against_its_restatement_under_sanitizers(tmp_path):
    """tests/c/hamming_plan_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: the scanned patterns (order, minus-strand bytes, N thresholds, dropped patterns), the launch
    groups for 1 .. 700 patterns and hamming_batch 0, 1, 2, 8, the tables of a group for m = 1 .. 1024 and hamming_items 0, 1,
    64, 300, the overflow step on the driver's own cases and on 20000 random chains, the text batches, hamming_count_copies,
    the popcount prefix."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hamming_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "hamming_plan_driver.cc")])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
        fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
        assert int(fields["tables"]) == 4 * 8 * 4 and int(fields["chains"]) == 20000
        assert int(fields["patterns"]) > 2000 and int(fields["groups"]) > 3 * 700 * 701 // 2 and int(fields["batches"]) > 400
