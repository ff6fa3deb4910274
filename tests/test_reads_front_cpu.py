"""CPU-only: the shared front of the read-batch calls (read_overlaps, merge_pairs, trim_reads, demux_reads, umi_groups_reads,
dedup_reads, reads_slice / reads_select).  Code and full message of every refusal the entry points raise before a batch is read
are compared EXACTLY with tests/golden/reads_front.json, recorded on the commit before the calls got one owner for their
refusals (tools/record_reads_front.py); reads_gate.h is walked alone by a stand-alone host program under AddressSanitizer /
UBSan; and each of the things the owner owns has one definition in sassy_amd/csrc."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sassy_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reads_front.json")


@pytest.fixture(scope="module")
def sassy():
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


def test_refusals_before_a_batch_is_read_are_the_recorded_ones(sassy):
    code = r'''
import json, os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "helpers"))
import sassy_amd, reads_front
print(json.dumps(reads_front.no_device(sassy_amd)))
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = json.loads(p.stdout)
    want = {e["call"]: e for e in json.load(open(GOLDEN))["no_device"]["refusals"]}
    assert len(got) >= 140 and len({e["call"] for e in got}) == len(got)
    for e in got:
        assert e["call"] in want, ("the golden file lacks", e["call"])
        assert e == want[e["call"]], (e, want[e["call"]])
    # all seven entry points, both codes, and every shared refusal that needs no batch
    assert {e["call"].split()[1] for e in got} == {"read_overlaps", "merge_pairs", "trim_reads", "demux_reads", "umi_groups_reads", "dedup_reads",
                                                   "reads_slice", "reads_select"}
    assert {e["rc"] for e in got} == {-1, -3}
    for word in ("use a dna or an iupac searcher", "does not take overhang", "only_best_match is not supported", "does not take max_n_frac",
                 "() must not be null"):
        assert sum(word in e["msg"] for e in got) >= 6, word


def test_the_gate_alone_under_sanitizers(tmp_path):
    """tests/c/reads_gate_driver.cc: a stand-alone program (its own main, no HIP) built with the host compiler and
    -fsanitize=address,undefined: the shared refusals in their order for one handle and for two, the bounded read length."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "reads_gate_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "c", "reads_gate_driver.cc")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    fields = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}
    assert fields == {"refusals": 15 + 18, "lengths": 2 * 5 * 8 * 11}, fields


def test_gate_header_is_free_of_hip_and_the_owner_has_one_of_each():
    src = open(os.path.join(CSRC, "reads_gate.h")).read()
    code = re.sub(r"//.*", "", src)
    assert "#include <hip" not in src and "hipStream" not in src and "getenv" not in src and "asm" not in code and "switch" not in code
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>", '#include "hamming_step.h"']
    for fn in ("reads_gate_searcher", "reads_gate_handles", "reads_fit_len"):
        assert len(re.findall(r"SASSY_HAM_HD \w+ " + fn + r"\(", src)) == 1, fn
    assert '#include "reads_gate.h"' in open(os.path.join(CSRC, "overlap_step.h")).read()
    driver = open(os.path.join(ROOT, "tests", "c", "reads_gate_driver.cc")).read()
    assert "int main(" in driver and "#include <hip" not in driver and "__global__" not in driver and "reads_gate.h" in driver
    # one definition each in sassy_amd/csrc: the searcher snapshot, the code of a shared refusal, the Dna look, the tickets' text
    # outside SASSY_NO_TICKETS, the bounded length
    units = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))}
    where = lambda text: sorted(f for f, body in units.items() if text in body)
    assert where("s->profile == PROFILE_DNA ? kHamDna") == ["reads_call.hip"] and units["reads_call.hip"].count("? kHamDna") == 1
    assert where("why == kRdsOverhang || why == kRdsOnlyBest || why == kRdsNFrac ? SASSY_HIP_EUNSUPPORTED") == ["reads_call.hip"]
    assert not [f for f, body in units.items() if re.search(r"k(Ovl|Trm|Dmx|Ddp)\w+ \? SASSY_HIP_EUNSUPPORTED", body)]
    assert where('which a dna searcher cannot "') == ["reads_call.hip"] and units["reads_call.hip"].count("which a dna searcher cannot") == 1
    assert where("finish them first") == ["host_internal.h", "multi_device.hip", "reads_call.hip"]
    assert units["reads_call.hip"].count("finish them first") == 1 and units["host_internal.h"].count("finish them first") == 1
    rule = re.compile(r"<= \w*\.?bytes && \w+ <= \w*\.?bytes - ")   # (the pair kernels judge both reads of a pair at once: bytes1, bytes2)
    assert sorted(f for f, body in units.items() if rule.search(body)) == ["reads_gate.h"] and len(rule.findall(units["reads_gate.h"])) == 1
    for f in ("trim_reads.hip", "demux_reads.hip", "dedup_reads.hip"):
        assert "reads_fit_len(" in units[f] and "TrmLoad16" in units[f] and "load16 = [&]" not in units[f], f
    for f in ("read_overlaps.hip", "merge_pairs.hip", "trim_reads.hip", "demux_reads.hip", "dedup_reads.hip"):
        assert "reads_gate_of(" in units[f] and "reads_gate_read(" in units[f] and "std::isnan" not in units[f] and "DeviceGuard" not in units[f], f
    for f in ("merge_pairs.hip", "trim_reads.hip", "demux_reads.hip", "dedup_reads.hip"):
        assert "reads_new_batch(" in units[f] and "unique_ptr" not in units[f] and "reset_stats" not in units[f] and "now_ms" not in units[f], f
    assert len(re.findall(r"\nint reads_new_batch\(", units["host_internal.h"])) == 1
    assert len(re.findall(r"\nint windows_from_host\(", units["reads_call.hip"])) == 1
    assert "windows_from_host(" in units["trim_reads.hip"] and "windows_from_host(" in units["demux_reads.hip"]
    build = open(os.path.join(ROOT, "sassy_amd", "build.py")).read()
    assert '"reads_call.hip"' in build and '"reads_gate.h"' in build
