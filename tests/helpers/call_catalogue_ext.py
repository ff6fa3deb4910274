"""Entries of the call catalogue (call_catalogue.py) for the Searcher calls that are inherited from its base classes, in
call_catalogue's own form -- cc.Entry objects whose run() and expect() return the same canonical value -- so that the
call-order tests can walk them against every entry of the catalogue.  The catalogue itself is only read: nothing here is
appended to cc.ENTRIES, and its counts stay what tests/test_call_catalogue_cpu.py pins.

tests/test_trim_reads_cpu.py checks that every public method a base class of Searcher defines is named by an entry here, the
guard test_call_catalogue_cpu.py keeps for the methods of Searcher itself; tests/test_gpu_trim_call_order.py walks them."""
import numpy as np

import call_catalogue as cc
import trim_reads_ref as tref

TRIM_FIELDS = (("length", "<u4"), ("quality_len", "<u4"), ("adapter_pos", "<u4"), ("adapter", "<i2"), ("overlap", "u1"), ("mismatches", "u1"))
TRIM_CALL = (4, 2, 100, 12, 20)   # min_overlap, k, max_permille, quality_cutoff, min_length


def trim_adapters(fx):
    """three 14-mers cut out of R1's own reads, so that some reads hold one whole and others a prefix of one at their end"""
    seqs = [x[0] for x in fx.d.pairs1 if len(x[0]) >= 60]
    return [seqs[0][30:44], seqs[1][-9:] + b"ACGTA", seqs[2][45:59]]


def _trim_expected(fx):
    return fx.memo("trim", lambda: tref.expected_trim(fx.profile, fx.d.pairs1, trim_adapters(fx), *TRIM_CALL))


def _trim_run(sassy, s, fx):
    trimmed, records = s.trim_reads(fx.dev.h1, trim_adapters(fx), *TRIM_CALL, with_records=True)
    try:
        return (cc.canon_struct(records, TRIM_FIELDS),) + cc.canon_handle(trimmed)
    finally:
        trimmed.free()


def _trim_expect(fx):
    records, seqs, quals = _trim_expected(fx)
    return (cc.canon_struct(records, TRIM_FIELDS),) + cc.expected_handle(seqs, quals)


def _trim_route(kind):
    # the Dna look where the searcher is a dna one, the find kernel, the three kernels of the layout scan, the write kernel
    return {"scan_launches": 6 if kind.alphabet == "dna" else 5, "word_rows": 8}


def _refusal(name, family, kinds, methods, call, words):
    def run(sassy, s, fx):
        try:
            call(sassy, s, fx)
        except sassy.SassyHipError as e:
            return tuple(w for w in words if w in str(e))
        return ("not refused",)
    return cc.Entry(name, family, kinds, methods, run, lambda fx: tuple(words), refusal=True)


ENTRIES = [
    cc.Entry("trim_reads", "reads", cc.NUC, ["trim_reads"], _trim_run, _trim_expect, route=_trim_route,
             size_of=lambda v: int(np.count_nonzero(np.frombuffer(v[0][4][-1], dtype="u1")))),   # the reads with an adapter found
    _refusal("refused_trim_ascii", "reads", cc.TEXTY, ["trim_reads"],
             lambda sassy, s, fx: s.trim_reads(fx.dev.h1, [b"ACGTAC"]), ("use a dna or an iupac searcher",)),
    _refusal("refused_trim_without_qualities", "reads", cc.NUC, ["trim_reads"],
             lambda sassy, s, fx: s.trim_reads(fx.dev.plain1, [b"ACGTAC"], quality_cutoff=20), ("KEEP_QUALITY",)),
]
assert not {e.name for e in ENTRIES} & {e.name for e in cc.ENTRIES}


def entries_for(kind):
    kid = kind.id if isinstance(kind, cc.Kind) else kind
    return [e for e in ENTRIES if kid in e.kinds]


_EXPECTED = {}


def expected(kind_id, name):
    key = (kind_id, name)
    if key not in _EXPECTED:
        _EXPECTED[key] = next(e for e in ENTRIES if e.name == name).expect(cc.KIND_FIXTURES(kind_id))
    return _EXPECTED[key]
