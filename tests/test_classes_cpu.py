"""No GPU: the host side of character-class patterns -- the cube cover (sassy_hip_class_cover), the expression parser
(sassy_amd.parse_classes) and the numpy reference the GPU tests compare against (helpers/classes_ref.py)."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

import oracle
import sassy_amd
from sassy_amd import ClassPattern, SassyHipError, parse_classes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import classes_ref as cref  # noqa: E402

MAX_SET_CUBES = 128  # include/sassy_hip.h: a set of n bytes takes at most n cubes, its complement at most 256 - n
MAX_RUN_CUBES = 14   # a run of consecutive byte values: 7 growing and 7 shrinking aligned power-of-two cubes


def set_bytes(members) -> bytes:
    b = bytearray(32)
    for c in members:
        b[c >> 3] |= 1 << (c & 7)
    return bytes(b)


class Cover:
    """sassy_hip_class_cover through ctypes with buffers reused over 35 000 calls."""

    def __init__(self):
        self.L = sassy_amd.lib()
        self.value = (C.c_uint8 * 128)()
        self.care = (C.c_uint8 * 128)()
        self.inv = C.c_int(0)
        self.all = np.arange(256, dtype=np.uint16)

    def __call__(self, set32: bytes):
        n = self.L.sassy_hip_class_cover(set32, self.value, self.care, 128, C.byref(self.inv))
        assert 0 <= n <= MAX_SET_CUBES, n
        v = np.frombuffer(self.value, dtype=np.uint8)[:n].astype(np.uint16)
        c = np.frombuffer(self.care, dtype=np.uint8)[:n].astype(np.uint16)
        inside = (((self.all[None, :] ^ v[:, None]) & c[:, None]) == 0).any(axis=0) if n else np.zeros(256, dtype=bool)
        if self.inv.value:
            inside = ~inside
        return n, bool(self.inv.value), np.packbits(inside, bitorder="little").tobytes()


@pytest.fixture(scope="module")
def cover():
    return Cover()


def test_cover_of_singletons_and_the_two_trivial_sets(cover):
    for c in range(256):
        n, inv, back = cover(set_bytes([c]))
        assert (n, inv, back) == (1, False, set_bytes([c])), c
    assert cover(bytes(32)) == (0, False, bytes(32))
    n, inv, back = cover(b"\xff" * 32)
    assert back == b"\xff" * 32 and n <= 1


def test_cover_of_every_range(cover):
    bits = np.zeros(256, dtype=bool)
    cases = 0
    for a in range(256):
        bits[:] = False
        for b in range(a, 256):
            bits[b] = True
            st = np.packbits(bits, bitorder="little").tobytes()
            n, inv, back = cover(st)
            assert back == st, (a, b)
            assert n <= MAX_RUN_CUBES, (a, b, n)
            cases += 1
    assert cases == 32896


def test_cover_of_random_sets_and_their_complements(cover):
    rng = random.Random(20261017)
    seen_inv = 0
    for i in range(1000):
        density = rng.choice((1, 2, 5, 20, 64, 128, 192, 250, 255))
        members = rng.sample(range(256), density)
        st = set_bytes(members)
        co = bytes(x ^ 0xFF for x in st)
        n, inv, back = cover(st)
        assert back == st, i
        n2, inv2, back2 = cover(co)
        assert back2 == co, i
        assert n <= min(density, 256 - density) and n2 <= min(density, 256 - density), (i, n, n2)
        seen_inv += inv + inv2
    assert seen_inv > 100


def test_cover_counts_without_buffers():
    L = sassy_amd.lib()
    assert L.sassy_hip_class_cover(set_bytes(range(3, 200)), None, None, 0, None) == 5
    cubes, inv = sassy_amd.class_cover(range(3, 200))
    assert inv and len(cubes) == 5


def members(p: ClassPattern):
    return [frozenset(p.members(j)) for j in range(p.m)]


DIGITS = frozenset(b"0123456789")
WORD = frozenset(b"0123456789_abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")
SPACE = frozenset(b" \t\n\r\f\v")
ALL = frozenset(range(256))


def test_parser_grammar():
    assert members(parse_classes(b"gr[ae]y")) == [{103}, {114}, {97, 101}, {121}]
    assert members(parse_classes(rb"\d\d-\D")) == [DIGITS, DIGITS, {45}, ALL - DIGITS]
    assert members(parse_classes(rb"\w\W\s\S")) == [WORD, ALL - WORD, SPACE, ALL - SPACE]
    assert members(parse_classes(b".")) == [ALL - {10}]
    assert members(parse_classes(b"[^ ]")) == [ALL - {32}]
    assert members(parse_classes(b"[a-cx-z0]")) == [frozenset(b"abcxyz0")]
    # a ']' right behind '[' or '[^' is a member; so is a '-' in front of the closing bracket
    assert members(parse_classes(b"[]]")) == [{93}]
    assert members(parse_classes(b"[]a]")) == [{93, 97}]
    assert members(parse_classes(b"[^]]")) == [ALL - {93}]
    assert members(parse_classes(b"[a-]")) == [{97, 45}]
    # escapes: \n \t \xHH and the escaped specials, inside and outside brackets
    assert members(parse_classes(rb"\n\t\x41\xfF")) == [{10}, {9}, {0x41}, {0xFF}]
    assert members(parse_classes(rb"\.\[\]\\\^\-")) == [{46}, {91}, {93}, {92}, {94}, {45}]
    assert members(parse_classes(rb"[\]\^\-\\]")) == [{93, 94, 45, 92}]
    assert members(parse_classes(rb"[\x00-\x1f\d_]")) == [frozenset(range(32)) | DIGITS | {95}]
    assert members(parse_classes(rb"[^\s\d]")) == [ALL - SPACE - DIGITS]
    # no quantifiers, alternation or anchors: those bytes are literals
    assert members(parse_classes(b"a*|$")) == [{97}, {42}, {124}, {36}]
    # bytes >= 0x80 and str input
    assert members(parse_classes(b"\xe9[\x80-\xff]")) == [{0xE9}, frozenset(range(128, 256))]
    assert parse_classes("ab") == parse_classes(b"ab")
    p = parse_classes(rb"\d\d\d\d-\d\d-\d\d")
    assert p.m == 10 and len(p.sets) == 320


def test_from_sets_and_layout():
    p = ClassPattern.from_sets([b"ab", [0, 255], []])
    assert p.m == 3 and members(p) == [{97, 98}, {0, 255}, frozenset()]
    assert p.sets[32 * 0 + (97 >> 3)] == (1 << (97 & 7)) | (1 << (98 & 7))
    assert p.sets[32] == 1 and p.sets[63] == 0x80 and p.sets[64:] == bytes(32)
    with pytest.raises(SassyHipError):
        ClassPattern.from_sets([[256]])
    with pytest.raises(SassyHipError):
        ClassPattern(b"\0" * 33)


@pytest.mark.parametrize("expr, offset", [
    (b"", 0),                # an empty expression
    (b"ab[cd", 2),           # an unterminated class
    (b"[", 0),
    (b"x[]", 1),             # (the ']' is a member: still open)
    (b"[z-a]", 1),           # a reversed range
    (b"ab[0-9][9-0]", 8),
    (b"abc\\", 3),           # a trailing backslash
    (b"[a\\", 2),
    (rb"\x4", 0),            # \x needs two hex digits
    (rb"\q", 0),             # an unknown escape
])
def test_parser_errors_name_the_offset(expr, offset):
    with pytest.raises(SassyHipError) as e:
        parse_classes(expr)
    assert ("offset %d" % offset) in str(e.value), str(e.value)


def test_case_closure_of_the_reference_helper():
    sets = members(parse_classes(b"a[B-D][^x]_1"))
    closed = cref.close_case(sets)
    # ([^x] holds 'X', whose twin closes the gap: under -i the complement of a letter is everything)
    assert closed == [frozenset(b"aA"), frozenset(b"BCDbcd"), ALL, {95}, {49}]
    # closing is idempotent and leaves '@' / '`', '[' / '{' alone
    assert cref.close_case(closed) == closed
    assert cref.close_case([frozenset(b"@["), frozenset(b"`{")]) == [frozenset(b"@["), frozenset(b"`{")]


def test_reference_last_row_with_singletons_is_the_ascii_oracle():
    rng = random.Random(5)
    text = bytes(rng.choice(b"abcde \n\xe9") for _ in range(3000))
    for m in (1, 7, 33, 70):
        at = rng.randrange(len(text) - m)
        pat = text[at:at + m]
        got = cref.last_row([frozenset([c]) for c in pat], text)
        assert (got == oracle.last_row("ascii", pat, text)).all(), m


IUPAC_SETS = {"A": b"A", "C": b"C", "G": b"G", "T": b"T", "R": b"AG", "Y": b"CT", "S": b"CG", "W": b"AT", "K": b"GT",
              "M": b"AC", "B": b"CGT", "D": b"AGT", "H": b"ACT", "V": b"ACG", "N": b"ACGT"}


def test_reference_last_row_with_base_sets_is_the_iupac_oracle():
    rng = random.Random(6)
    text = bytes(rng.choice(b"ACGT") for _ in range(4000))
    codes = "".join(IUPAC_SETS)
    for m in (4, 20, 45):
        pat = "".join(rng.choice(codes) for _ in range(m))
        got = cref.last_row([frozenset(IUPAC_SETS[c]) for c in pat], text)
        assert (got == oracle.last_row("iupac", pat.encode(), text)).all(), pat
        assert int(got.min()) < m  # the comparison sees costs below the trivial one


def test_symbols_are_exported():
    assert "sassy_hip_search_classes" in sassy_amd.EXPORTED_SYMBOLS and "sassy_hip_class_cover" in sassy_amd.EXPORTED_SYMBOLS
    L = sassy_amd.lib()
    assert L.sassy_hip_search_classes and L.sassy_hip_class_cover
    assert sassy_amd.CLASS_MAX_CUBES == 256
