"""The call catalogue (tests/helpers/call_catalogue.py) checked without a device: every public entry point of
sassy_amd.Searcher is catalogued or excluded with a reason -- a new entry point fails here until it has an entry --, every
expectation is non-trivial, the probing pairs really differ, and all expectations together are cheap to build.

Measured: building all 419 (kind, entry) expectations takes 11 s here on 16 threads (19 s on one); the bound is 60 s."""
import inspect
import os
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import call_catalogue as cc  # noqa: E402
import classes_ref as cref  # noqa: E402
import oracle  # noqa: E402

EXEMPT_PREFIXES = ("set_", "with_", "get_", "enable_", "_")
# public methods that are no call of the catalogue, each with its reason
EXCLUDED = {
    "format_tsv": "formats one finished Match on the host: no device work, no searcher state is read or written",
    "stats": "reads the last call's statistics; tests/test_gpu_call_order.py::test_stats_are_the_last_calls checks it after every entry",
}


@pytest.fixture(scope="module")
def built():
    """all expectations, and how long they took (the first thing this module does with the catalogue)"""
    t0 = time.time()
    n = cc.build_all_expectations(threads=16)
    return n, time.time() - t0


def test_building_all_expectations_takes_under_60_seconds(built):
    n, seconds = built
    print("built %d expectations in %.1f s" % (n, seconds))
    assert n == sum(len(cc.entries_for(k)) for k in cc.KINDS) and n > 400
    assert seconds < 60.0, seconds


def test_every_public_method_is_catalogued_or_excluded():
    import sassy_amd
    public = [name for name, f in vars(sassy_amd.Searcher).items() if inspect.isfunction(f) and not name.startswith(EXEMPT_PREFIXES)]
    assert len(public) >= 38 and "search" in public and "merge_pairs" in public and "stats" in public
    named = {m for e in cc.ENTRIES for m in e.methods}
    missing = [m for m in public if m not in named and m not in EXCLUDED]
    assert not missing, "Searcher methods without a catalogue entry (tests/helpers/call_catalogue.py) or an EXCLUDED reason: %s" % missing
    # the catalogue names real methods only, and nothing is both catalogued and excluded
    assert not [m for m in named if not hasattr(sassy_amd.Searcher, m)]
    assert not [m for m in EXCLUDED if m in named or m not in public]
    assert all(len(reason) > 20 for reason in EXCLUDED.values())


def test_every_entry_runs_for_a_kind_and_names_are_unique():
    names = [e.name for e in cc.ENTRIES]
    assert len(set(names)) == len(names)
    ids = {k.id for k in cc.KINDS}
    for e in cc.ENTRIES:
        assert e.kinds and set(e.kinds) <= ids, e
        assert e.family and e.methods and callable(e.expect), e
        assert (e.results is not None) != (e._run is not None), e
    for k in cc.KINDS:
        assert len(cc.entries_for(k)) >= 18, k
    # every family with a big sibling names a small one of the same family and kinds
    bigs = [e for e in cc.ENTRIES if e.big]
    assert sorted({e.family for e in bigs}) == ["hamming", "overlaps", "scan", "sets", "umi"]
    for e in bigs:
        small = cc.by_name(e.small)
        assert not small.big and small.family == e.family and set(e.kinds) <= set(small.kinds), e


def test_every_expectation_is_non_trivial(built):
    for k in cc.KINDS:
        for e in cc.entries_for(k):
            want = cc.expected(k.id, e.name)
            hash(want)  # canonical values are hashable
            if e.refusal:
                assert want and all(isinstance(w, str) and w for w in want), (k.id, e.name)
            else:
                assert e.size_of(want) >= 1, (k.id, e.name, "expects no match, record or merged pair")
    # what the big siblings are for
    assert cc.expected("dna", "search_all_poly_a_70000")[0][1] > 65536
    assert cc.expected("dna", "search_hamming_20000_hits")[0][1] == 20000
    assert len(cc.data().set_big) == 3000 and len(cc.data().big_r1) == 1100 and max(map(len, cc.data().big_r1)) == 512
    for t in (cc.data().t1, cc.data().t2, cc.data().seeded_text, cc.data().big_text, cc.data().fastq, cc.data().fasta):
        assert len(t) < (1 << 20)
    assert len(cc.data().t1) == 6144 and len(cc.data().t2) == 40960
    assert len(cc.expected("dna", "search")) == 5   # the five planted near-matches of T1


def test_the_probing_pairs_differ(built):
    probes = 0
    for k in cc.KINDS:
        for e in cc.entries_for(k):
            if e.twin:   # the same length, other bytes
                other = cc.by_name(e.twin)
                assert cc.expected(k.id, e.name) != cc.expected(k.id, e.twin), (k.id, e.name)
                assert len(cc.data().p20) == len(cc.data().p20b) and cc.data().p20 != cc.data().p20b and other.family == e.family
                probes += 1
            if e.plain:  # a reporting mode against the plain call on the same inputs
                assert k.id in cc.by_name(e.plain).kinds, (k.id, e.name)
                assert cc.expected(k.id, e.name) != cc.expected(k.id, e.plain), (k.id, e.name, "the mode changes nothing")
                probes += 1
    assert probes >= 7 + 4 + 6 + 2
    # another k on the same pattern gives another result as well
    assert cc.expected("dna", "search_other_k") != cc.expected("dna", "search")
    # the rewritten device text: its two contents give different results
    first, second = cc.expected("dna", "search_device_text_rewritten")
    assert first != second


@pytest.mark.parametrize("kind_id", cc.TEXTY)
def test_the_class_entrys_expectation_is_the_class_definition(kind_id):
    """search_classes' expectation is the oracle's on a mapped text; classes_ref's DP row under set membership gives the same
    ends and costs, and every record replays as an alignment under the sets."""
    import sassy_amd
    cp = sassy_amd.parse_classes(cc.CLASS_EXPR)
    sets = [frozenset(cp.members(j)) for j in range(cp.m)]
    if kind_id == "ascii_ci":
        sets = cref.close_case(sets)
    text = cc.data().t1_class
    want = cc.expected(kind_id, "search_classes")
    ends = oracle.find_ends(cref.last_row(sets, text), 2)
    assert sorted((r[3], r[6]) for r in want) == sorted(ends) and len(want) >= 2
    for r in want:
        cref.replay(sets, text, oracle.Match(r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]))
    # ... and the two plants that carry X / Y are among them
    assert {200, 1400} <= {r[2] for r in want}


def test_the_matrix_is_what_the_documents_say():
    """entries per kind, and the ordered pairs (B, A) that test_gpu_call_order.py::test_after_every_other_call runs: every
    non-big entry as A against every other entry of its kind as B"""
    per_kind = {k.id: len(cc.entries_for(k)) for k in cc.KINDS}
    assert per_kind == {"dna": 73, "dna-rc": 72, "iupac": 74, "iupac-rc": 74, "iupac-alpha": 18, "ascii": 54, "ascii_ci": 54}, per_kind
    pairs = sum(len([e for e in cc.entries_for(k) if not e.big]) * (len(cc.entries_for(k)) - 1) for k in cc.KINDS)
    assert pairs == 25333, pairs
