"""search_all_alignments without a device: the CPU checker against the reference's asserted values and against its own
brute-force mode, the C-ABI / Python surface, and the loud failure without a device."""
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import all_alignments_ref as ref  # noqa: E402


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "all_alignments.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    return sassy_amd


@pytest.mark.parametrize("entry", _golden(), ids=lambda e: e["name"])
def test_checker_reproduces_reference_assertions(entry):
    groups = ref.search_all_alignments(entry["alphabet"], entry["pattern"].encode(), entry["text"].encode(), entry["k"],
                                       rc=entry["rc"], max_n_frac=entry["max_n_frac"])
    ref.check_golden(entry, groups)


def test_checker_dfs_equals_brute_force():
    """The DFS checker and the unpruned enumeration filtered by the rules agree as sets, group by group."""
    rng = random.Random(20261015)
    alphabets = {"dna": b"ACGT", "iupac": b"ACGTN", "ascii": b"ab"}
    cases = 0
    for _ in range(400):
        prof = rng.choice(list(alphabets))
        letters = alphabets[prof]
        if prof == "iupac":
            pat = bytes(rng.choice(b"ACGTRY") for _ in range(rng.randint(1, 6)))
        else:
            pat = bytes(rng.choice(letters) for _ in range(rng.randint(1, 6)))
        text = bytes(rng.choice(letters) for _ in range(rng.randint(0, 10)))
        k = rng.randint(0, 3)
        rc = prof != "ascii" and rng.random() < 0.5
        a = ref.search_all_alignments(prof, pat, text, k, rc=rc)
        b = ref.search_all_alignments(prof, pat, text, k, rc=rc, brute=True)
        assert [sorted(g) for g in a] == [sorted(g) for g in b], (prof, pat, text, k, rc)
        assert all(len(set(g)) == len(g) for g in a)
        cases += bool(a)
    assert cases > 100


def test_checker_rc_equals_fwd_on_reverse_complement():
    """The reference's search_all_alignments_rc_fuzz property, on the checker."""
    rng = random.Random(42)
    import oracle
    for _ in range(60):
        plen = rng.randint(4, 12)
        pat = bytes(rng.choice(b"ACGT") for _ in range(plen))
        text = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(plen, plen + 8)))
        k = rng.randint(0, 3)
        n = len(text)
        rc = [x for g in ref.search_all_alignments("dna", pat, text, k, rc=True) for x in g if x[5] == "-"]
        fwd = [x for g in ref.search_all_alignments("dna", pat, oracle.reverse_complement("dna", text), k) for x in g]
        assert sorted((x[0], x[1], x[4], x[6]) for x in rc) == sorted((n - x[1], n - x[0], x[4], x[6]) for x in fwd)


def test_symbol_declared_exported_and_bound(sassy):
    import re
    hdr = open(os.path.join(ROOT, "include", "sassy_hip.h")).read()
    assert re.search(r"\bsassy_hip_search_all_alignments\s*\(", hdr)
    assert "sassy_hip_search_all_alignments" in sassy.EXPORTED_SYMBOLS
    assert hasattr(sassy.lib(), "sassy_hip_search_all_alignments")
    assert callable(getattr(sassy.Searcher, "search_all_alignments", None))
    assert "aa_batch" in [r[0] for r in sassy.option_table()]


def test_search_all_alignments_without_device_fails_loudly():
    """A child process that sees no HIP device: ENODEVICE, no result from anywhere else; bad flags and overhang
    searchers are refused before any device work."""
    code = (
        "import re, sassy_amd\n"
        "def raises(pattern, f, *args):\n"
        "    try:\n"
        "        f(*args)\n"
        "    except sassy_amd.SassyHipError as e:\n"
        "        assert re.search(pattern, str(e)), e\n"
        "    else:\n"
        "        raise AssertionError('no SassyHipError: ' + pattern)\n"
        "assert sassy_amd.device_count() == 0, sassy_amd.device_count()\n"
        "s = sassy_amd.Searcher('dna', rc=True)\n"
        "raises('error -2: no usable HIP device', s.search_all_alignments, b'ACGT', b'ACGTACGT', 1)\n"
        "raises('error -3: .*overhang', sassy_amd.Searcher('iupac', rc=False, alpha=0.5).search_all_alignments,"
        " b'ACGT', b'ACGT', 1)\n"
        "import ctypes as C\n"
        "out = C.c_void_p()\n"
        "rc = sassy_amd.lib().sassy_hip_search_all_alignments(s._h, b'ACGT', 4, C.c_char_p(b'ACGT'), 4, 0,"
        " sassy_amd.ALL_MINIMA, C.byref(out))\n"
        "assert rc == -1 and not out.value, rc\n"
        "print('ok')\n"
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
