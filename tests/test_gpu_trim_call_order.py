"""Call order: a trim between two calls of other families on ONE searcher changes neither's result, and the trim's own result
does not depend on what ran in front of it.  The trim keeps its records and its adapter table in buffers of the searcher and
runs the Dna look and the layout scan on the searcher's stream, which the other families use as well."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import read_overlaps_ref as oref  # noqa: E402
import trim_reads_ref as tref  # noqa: E402

pytestmark = pytest.mark.gpu

AD = b"AGATCGGAAGAGCACACGTC"


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


def test_a_trim_between_calls_of_other_families(sassy):
    rng = np.random.default_rng(6)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = []
    for i in range(50):
        n = int(rng.integers(40, 150))
        s = bytearray(bytes(rng.choice(letters, n).astype(np.uint8)))
        if i % 3:
            c = int(rng.integers(10, n))
            s[c:] = (AD + bytes(s[c:]))[:n - c]
        seqs.append(bytes(s))
    reads = [(s, bytes(rng.integers(33, 75, len(s)).astype(np.uint8))) for s in seqs]
    mates = [oref.revcomp("dna", s[-30:]) for s in seqs]
    pats = [seqs[0][3:15], seqs[7][10:22], b"ACGTACGTACGT"]
    text = b"".join(seqs)
    key = lambda m: (m.pattern_idx, getattr(m, "text_idx", 0), m.text_start, m.text_end, m.cost, m.strand, m.cigar)  # noqa: E731
    want = tref.expected_trim("dna", reads, [AD], 4, 2, 100, 15, 20)

    def trim(s):
        trimmed, records = s.trim_reads(reads, [AD], 4, 2, 100, 15, 20, with_records=True)
        out = (records.tobytes(), trimmed.download_text(), trimmed.download_quality_text(), trimmed.download_rem().tobytes())
        trimmed.free()
        return out

    families = {
        "search": lambda s: [key(m) for m in s.search(pats[0], text, 1)],
        "search_many": lambda s: [key(m) for m in s.search_many(pats, seqs, 2)],
        "hamming_best_pattern": lambda s: [a.tolist() for a in s.hamming_best_pattern(pats, seqs, 2)],
        "read_overlaps": lambda s: s.read_overlaps(seqs, mates, 10, 2, 100).tobytes(),
        "merge_pairs": lambda s: (lambda m: (m.download_text(), m.free())[0])(s.merge_pairs(reads, [(m, b"I" * len(m)) for m in mates], 10, 2, 100)),
    }
    fresh = {name: fn(sassy.Searcher("dna", rc=False)) for name, fn in families.items()}
    alone = trim(sassy.Searcher("dna", rc=False))
    assert alone[0] == want[0].tobytes() and (want[0]["adapter"] >= 0).sum() > 25
    assert len(fresh["search_many"]) > 2 and len(fresh["search"]) > 0
    names = list(families)
    for i, before in enumerate(names):
        after = names[(i + 1) % len(names)]
        s = sassy.Searcher("dna", rc=False)
        assert families[before](s) == fresh[before], before
        assert trim(s) == alone, ("the trim behind", before)
        assert families[after](s) == fresh[after], (after, "behind a trim")
        assert families[before](s) == fresh[before], (before, "again")
        assert trim(s) == alone, ("the trim again, behind", before)


# ================================================================ against the call catalogue
# Searcher.trim_reads is inherited from a base class of Searcher, so tests/helpers/call_catalogue.py does not list it and
# tests/test_gpu_call_order.py does not walk it.  Its entries are tests/helpers/call_catalogue_ext.py's, in the catalogue's form,
# and the tests below are that file's for them: each alone on its route, each as A through every other entry B, and each as B
# in the row of every entry A of the catalogue.  The catalogue is only read.
import call_catalogue as cc  # noqa: E402
import call_catalogue_ext as ext  # noqa: E402

STATS_FIELDS = ("text_bytes", "scan_launches", "candidates", "blocks", "word_rows")
EXT = [(k.id, e.name) for k in cc.KINDS for e in ext.entries_for(k)]
ROWS = [(k.id, a.name) for k in cc.KINDS if ext.entries_for(k) for a in cc.entries_for(k) if not a.big]


@pytest.fixture(scope="module")
def dev(sassy):
    side = cc.DeviceSide(sassy)
    yield side
    side.close()


@pytest.fixture(scope="module", autouse=True)
def expectations():
    cc.build_all_expectations()


def fixtures(kind_id, dev):
    fx = cc.KIND_FIXTURES(kind_id)
    fx.dev = dev
    return fx


def by_name(name):
    return next((e for e in ext.ENTRIES if e.name == name), None) or cc.by_name(name)


def check(sassy, s, fx, e, ctx):
    want = ext.expected(fx.kind.id, e.name) if e in ext.ENTRIES else cc.expected(fx.kind.id, e.name)
    got = e.run(sassy, s, fx)
    assert got == want, "%s: %s differs from its expectation" % (ctx, e.name)


def test_the_extension_names_the_trim_for_every_kind_that_has_it():
    assert sorted({k for k, _ in EXT}) == sorted(cc.PLAIN) and len(EXT) == 2 * len(cc.NUC) + len(cc.TEXTY)
    assert len(ROWS) > 200


@pytest.mark.parametrize("kind_id,name", EXT, ids=["%s-%s" % c for c in EXT])
def test_each_call_alone(sassy, dev, kind_id, name):
    """A fresh searcher, one call, equal to expect(), non-trivial, and on the route the entry is meant to take."""
    fx, e = fixtures(kind_id, dev), by_name(name)
    s = cc.make_searcher(sassy, fx.kind)
    check(sassy, s, fx, e, (kind_id, "alone"))
    want = ext.expected(kind_id, name)
    assert (all(w for w in want) and want) if e.refusal else e.size_of(want) >= 3, (kind_id, name)
    route = e.route(fx.kind)
    if route:
        st = s.stats()
        assert {f: st[f] for f in route} == route, (kind_id, name, "took another route", {f: st[f] for f in STATS_FIELDS})


@pytest.mark.parametrize("kind_id,name", EXT, ids=["%s-%s" % c for c in EXT])
def test_after_every_other_call(sassy, dev, kind_id, name):
    """One fresh searcher runs A, B1, A, B2, A ... over every other entry B of the kind, the catalogue's and the
    extension's; every result is checked, and what stats() says after A is the same every time."""
    fx, a = fixtures(kind_id, dev), by_name(name)
    s = cc.make_searcher(sassy, fx.kind)
    check(sassy, s, fx, a, (kind_id, "first call"))
    alone = {f: s.stats()[f] for f in STATS_FIELDS}
    prev = None
    for b in cc.entries_for(fx.kind) + ext.entries_for(fx.kind):
        if b is a:
            continue
        check(sassy, s, fx, b, "kind %s, order (previous B %s, A %s, B %s), as B" % (kind_id, prev, a.name, b.name))
        check(sassy, s, fx, a, "kind %s, order (previous B %s, B %s, A %s), as A" % (kind_id, prev, b.name, a.name))
        if not a.refusal:
            assert {f: s.stats()[f] for f in STATS_FIELDS} == alone, (kind_id, a.name, "stats behind", b.name)
        prev = b.name


@pytest.mark.parametrize("kind_id,name", ROWS, ids=["%s-%s" % c for c in ROWS])
def test_in_the_row_of_every_entry_of_the_catalogue(sassy, dev, kind_id, name):
    """The extension's entries as B in the row of a catalogue entry A, as tests/test_gpu_call_order.py would run them: one fresh
    searcher runs A, X1, A, X2, A over the extension's entries X of the kind."""
    fx, a = fixtures(kind_id, dev), cc.by_name(name)
    s = cc.make_searcher(sassy, fx.kind)
    check(sassy, s, fx, a, (kind_id, "first call"))
    for x in ext.entries_for(fx.kind):
        check(sassy, s, fx, x, "kind %s, order (A %s, B %s), as B" % (kind_id, a.name, x.name))
        check(sassy, s, fx, a, "kind %s, order (B %s, A %s), as A" % (kind_id, x.name, a.name))
