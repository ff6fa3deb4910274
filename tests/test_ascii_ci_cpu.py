"""CPU-only: the case-insensitive Ascii profile's host side -- the alphabet name is accepted wherever "ascii" is, the
searcher behaves like an ascii one where no device is needed, and without a device its searches fail loudly."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sassy():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import sassy_amd
    return sassy_amd


def test_ascii_ci_is_an_alphabet(sassy):
    for name in ("ascii_ci", "ASCII_CI", "Ascii_Ci"):
        s = sassy.Searcher(name, rc=False)
        assert s.alphabet == "ascii_ci"
    # the drop-in constructor and the multi-device one take the name as well
    L = sassy.lib()
    h = L.sassy_searcher(b"ascii_ci", False, float("nan"))
    assert h
    L.sassy_searcher_free(h)
    with pytest.raises(sassy.SassyHipError, match="Unsupported alphabet"):
        sassy.Searcher("protein")
    with pytest.raises(sassy.SassyHipError, match="Unsupported alphabet"):
        sassy.Searcher("ascii_cs")


def test_ascii_ci_refuses_what_ascii_refuses(sassy):
    # overhang: Iupac only
    with pytest.raises(sassy.SassyHipError, match="[Oo]verhang"):
        sassy.Searcher("ascii_ci", rc=False, alpha=0.5)
    # no complement: the searcher constructs, its first search fails (before any device work)
    s = sassy.Searcher("ascii_ci", rc=True)
    with pytest.raises(sassy.SassyHipError, match="reverse complement is not defined"):
        s.search(b"abc", b"xxABCxx", 0)
    with pytest.raises(sassy.SassyHipError, match="reverse complement is not defined"):
        s.search_many([b"abc"], [b"xxABCxx"], 0)
    with pytest.raises(sassy.SassyHipError, match="reverse complement is not defined"):
        s.best_matches([b"abc"], [b"xxABCxx"], 0)


def test_seed_layout_takes_the_name(sassy):
    """sassy_hip_seed_layout (host arithmetic) reads the name through the searchers' parser: ascii_ci cuts like ascii, in
    any letter case."""
    pats = [b"abcdefghijklmnopqrstuvw"] * 3
    assert sassy.seed_layout("ascii_ci", pats, 3) == sassy.seed_layout("ascii", pats, 3)
    assert sassy.seed_layout("ASCII_CI", pats, 3) == sassy.seed_layout("Ascii", pats, 3) == sassy.seed_layout("ascii", pats, 3)


def test_cli_alphabet_option_takes_the_name():
    sys.path.insert(0, ROOT)
    import argparse
    from sassy_amd.cli import add_search_arguments
    ap = argparse.ArgumentParser()
    add_search_arguments(ap)
    assert ap.parse_args(["-k", "1", "-p", "x", "-a", "ASCII_CI"]).alphabet == "ascii_ci"
    assert ap.parse_args(["-k", "1", "-p", "x", "-a", "ascii"]).alphabet == "ascii"
    assert ap.parse_args(["-k", "1", "-p", "x"]).alphabet == "iupac"


def test_ascii_ci_without_a_device_fails_loudly(sassy):
    """In a child process that sees no HIP device, as test_no_device_fails_loudly: no fallback for the new profile or
    the line resolution."""
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
        "s = sassy_amd.Searcher('ascii_ci', rc=False)\n"
        "raises('no usable HIP device', s.search, b'hello', b'say HELLO world', 1)\n"
        "raises('no usable HIP device', s.search_many, [b'hello'], [b'say HELLO world'], 1)\n"
        "raises('no usable HIP device', s.line_spans, b'a\\nb', [0], [2])\n"
        "raises('no usable HIP device', s.search_lines, b'hello', b'say\\nHELLO world', 1)\n"
        "print('ok')\n"
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
