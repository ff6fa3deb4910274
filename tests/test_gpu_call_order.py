"""Call order: one searcher through every entry point of the catalogue (tests/helpers/call_catalogue.py), in every order of
two, up and down the sizes, and along seeded walks.  A searcher keeps state between calls -- upload caches that decide "same
as last time", the twin control blocks, history-dependent routing, some sixty grow-only device buffers that the families
share or size differently (DESIGN.md names them) --, and every other GPU test runs its family on a searcher that has done
nothing else.  Every comparison here is exact equality with the catalogue's expectation, computed on the host once.

A failure names the searcher kind and the order -- (previous B, B, A) -- so that the pair can be rerun by hand:

    s = cc.make_searcher(sassy_amd, cc.KIND[kind]); fx = cc.KIND_FIXTURES(kind); fx.dev = cc.DeviceSide(sassy_amd)
    for name in (B, A): assert cc.by_name(name).run(sassy_amd, s, fx) == cc.expected(kind, name)

Wall time on an MI355X (pytest --durations=0): 38 s for the whole file -- 831 test ids, 25 333 ordered pairs; 4.5 s of it the
module's set-up, which builds the expectations; the slowest test id 0.25 s (a size ladder), a walk of 900 calls 0.2 s, a row
of the pair matrix 0.1 s.  The bound is 60 s; if it ever does not fit, WALK_CALLS and WALK_SEEDS give way, never the
catalogue or the pair matrix."""
import collections
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import call_catalogue as cc  # noqa: E402

pytestmark = pytest.mark.gpu

WALK_SEEDS = (11, 12, 13, 14, 15, 16)
WALK_CALLS = 150
KEPT_RESULTS = 20   # more than PinPool::kMaxAdopted (16): the newest kept results were copied out, the oldest adopted

# sassy_hip_Stats fields that include/sassy_hip.h documents as the LAST call's; what is left out, and why:
#   scan_ms, trace_ms, total_ms, filter_ms, host_enqueue_ms, host_wait_ms, host_post_ms   times
# and one entry is left out as A: line_spans is no search -- it reports through sassy_hip_line_span_times and leaves the last
# search's statistics in place, so what stats() says after it depends on the call before it
STATS_NOT_A_SEARCH = ("line_spans",)
STATS_FIELDS = ("text_bytes", "scan_launches", "candidates", "cond_resolved", "chunks", "blocks", "word_rows", "blocks_per_chunk",
                "warmup_blocks", "grid", "filtered", "hit_blocks", "piece_len", "fused", "live_blocks", "pair", "pass_patterns", "plane_launches")
STATS_ALONE = {}   # (kind, entry) -> the fields after the call alone on a fresh searcher (filled by test_each_call_alone)


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    if sassy_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return sassy_amd


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


def describe(got, want):
    """where two canonical values part, in a line"""
    if type(got) is not type(want):
        return "got %s, want %s" % (repr(got)[:200], repr(want)[:200])
    if isinstance(got, tuple):
        if len(got) != len(want):
            extra = [x for x in got if x not in want][:2] if len(got) < 10000 else []
            lost = [x for x in want if x not in got][:2] if len(want) < 10000 else []
            return "%d items, want %d; not wanted %s; missing %s" % (len(got), len(want), repr(extra)[:300], repr(lost)[:300])
        for i, (g, w) in enumerate(zip(got, want)):
            if g != w:
                return "item %d: %s" % (i, describe(g, w))
    if isinstance(got, bytes) and len(got) == len(want):
        at = next(i for i in range(len(got)) if got[i] != want[i])
        return "byte %d of %d: got %d, want %d" % (at, len(got), got[at], want[at])
    return "got %s, want %s" % (repr(got)[:200], repr(want)[:200])


def device_error(sassy, e):
    """a HIP runtime error ends the session: nothing more is started on a device that has faulted"""
    if isinstance(e, sassy.SassyHipError) and "error -2" in str(e):
        pytest.exit("HIP runtime error, stopping the session: %s" % e, returncode=3)


def check(sassy, s, fx, e, ctx):
    try:
        got = e.run(sassy, s, fx)
    except Exception as err:
        device_error(sassy, err)
        pytest.fail("%s: %s raised %s: %s" % (ctx, e.name, type(err).__name__, err))
    want = cc.expected(fx.kind.id, e.name)
    if got != want:
        pytest.fail("%s: %s differs from its expectation: %s" % (ctx, e.name, describe(got, want)))


def stats_of(s):
    st = s.stats()
    return {f: st[f] for f in STATS_FIELDS}


ALONE = [(k.id, e.name) for k in cc.KINDS for e in cc.entries_for(k)]
FIRST = [(k.id, e.name) for k in cc.KINDS for e in cc.entries_for(k) if not e.big]


@pytest.mark.parametrize("kind_id,name", ALONE, ids=["%s-%s" % c for c in ALONE])
def test_each_call_alone(sassy, dev, kind_id, name):
    """A fresh searcher, one call, equal to expect() -- and on the route the entry is meant to take, so that a wrong
    catalogue entry is not read as an order bug."""
    fx, e = fixtures(kind_id, dev), cc.by_name(name)
    s = cc.make_searcher(sassy, fx.kind)
    check(sassy, s, fx, e, (kind_id, "alone"))
    st = s.stats()
    route = e.route(fx.kind)
    if route:
        assert {f: st[f] for f in route} == route, (kind_id, name, "took another route", {f: st[f] for f in STATS_FIELDS})
    STATS_ALONE[(kind_id, name)] = {f: st[f] for f in STATS_FIELDS}


@pytest.mark.parametrize("kind_id,name", FIRST, ids=["%s-%s" % c for c in FIRST])
def test_after_every_other_call(sassy, dev, kind_id, name):
    """One fresh searcher runs A, B1, A, B2, A ... over every other entry B of the kind; every result is checked."""
    fx, a = fixtures(kind_id, dev), cc.by_name(name)
    s = cc.make_searcher(sassy, fx.kind)
    check(sassy, s, fx, a, (kind_id, "first call"))
    prev = None
    for b in cc.entries_for(fx.kind):
        if b is a:
            continue
        check(sassy, s, fx, b, "kind %s, order (previous B %s, A %s, B %s), as B" % (kind_id, prev, a.name, b.name))
        check(sassy, s, fx, a, "kind %s, order (previous B %s, B %s, A %s), as A" % (kind_id, prev, b.name, a.name))
        prev = b.name


@pytest.mark.parametrize("kind_id", [k.id for k in cc.KINDS if k.id != "iupac-alpha"])
def test_size_ladders(sassy, dev, kind_id):
    """Per family with a big sibling: small, big, small, big, small on one searcher -- every buffer of the family grows under
    the big call and is then used by the small one.  Across families: big scan, small Hamming, small pairs and the two
    rotations of that order."""
    fx = fixtures(kind_id, dev)
    bigs = [e for e in cc.entries_for(fx.kind) if e.big]
    assert len(bigs) >= 4
    for big in bigs:
        small = cc.by_name(big.small)
        s = cc.make_searcher(sassy, fx.kind)
        for step, e in enumerate((small, big, small, big, small)):
            check(sassy, s, fx, e, "kind %s, ladder %s / %s, step %d" % (kind_id, small.name, big.name, step))
    trio = [cc.by_name("search_all_poly_a_70000"), cc.by_name("search_hamming_host"), cc.by_name("hamming_pairs")]
    for r in range(3):
        order = trio[r:] + trio[:r]
        s = cc.make_searcher(sassy, fx.kind)
        for e in order + order:
            check(sassy, s, fx, e, "kind %s, across families %s" % (kind_id, [x.name for x in order]))


def walk_setters(sassy):
    """the setters that must not change any result, as (label, function of a searcher)"""
    out = [("set_fused(%d)" % v, lambda s, v=v: s.set_fused(bool(v))) for v in (0, 1)]
    out += [("set_prefilter(%d)" % v, lambda s, v=v: s.set_prefilter(v)) for v in (-1, 0, 1)]
    out += [("set_timing(%d)" % v, lambda s, v=v: s.set_timing(v)) for v in (0, 1, 2)]
    out += [("set_geometry_tuner(%d)" % v, lambda s, v=v: s.set_geometry_tuner(bool(v))) for v in (0, 1)]
    out += [("set_pipe_depth(%d)" % v, lambda s, v=v: s.set_pipe_depth(v)) for v in (1, 2, 4)]
    listed = {name for name, _, _ in sassy.option_table()}
    for name in ("shared_pass", "plane_cache"):
        assert name in listed, name
        out += [("set_option(%s, %d)" % (name, v), lambda s, name=name, v=v: s.set_option(name, v)) for v in (0, 1)]
    return out


def compare_kept(sassy, kept, ctx):
    for name, i, r, want in kept:
        got = cc.canon_result(sassy, r)
        if got != want:
            pytest.fail("%s: a kept result of %s (result %d) changed: %s" % (ctx, name, i, describe(got, want)))


@pytest.mark.parametrize("kind_id", [k.id for k in cc.KINDS])
def test_seeded_walks(sassy, dev, kind_id):
    """Six fixed seeds, 150 calls each, drawn from the non-big entries, on ONE searcher; between calls, with probability 1/4,
    a setter that must not change any result.  The last 20 Result objects stay alive and are compared again at the end of
    every walk, and once more when the searcher is gone."""
    fx = fixtures(kind_id, dev)
    pool = [e for e in cc.entries_for(fx.kind) if not e.big]
    setters = walk_setters(sassy)
    s = cc.make_searcher(sassy, fx.kind)
    kept = collections.deque(maxlen=KEPT_RESULTS)
    for seed in WALK_SEEDS:
        rng = random.Random(seed)
        log = collections.deque(maxlen=8)
        for step in range(WALK_CALLS):
            if rng.random() < 0.25:
                label, setter = rng.choice(setters)
                setter(s)
                log.append(label)
            e = rng.choice(pool)
            log.append(e.name)
            ctx = "kind %s, walk seed %d, call %d, after %s" % (kind_id, seed, step, list(log)[:-1])
            if e.results is None:
                check(sassy, s, fx, e, ctx)
                continue
            try:
                results = e.results(sassy, s, fx)
            except Exception as err:
                device_error(sassy, err)
                pytest.fail("%s: %s raised %s: %s" % (ctx, e.name, type(err).__name__, err))
            want = cc.expected(kind_id, e.name)
            got = cc.canon_results(sassy, results)
            if got != want:
                pytest.fail("%s: %s differs from its expectation: %s" % (ctx, e.name, describe(got, want)))
            for i, r in enumerate(results):
                kept.append((e.name, i, r, want[i]))
        compare_kept(sassy, kept, "kind %s, end of walk seed %d" % (kind_id, seed))
    assert len(kept) == KEPT_RESULTS
    del s
    compare_kept(sassy, kept, "kind %s, after the searcher was dropped" % kind_id)


def test_handles_outlive_their_makers(sassy, dev):
    """A merged batch needs neither its parents nor the searcher that made it; one read batch serves searchers of different
    profiles in turn."""
    d = cc.data()
    fx = fixtures("dna", dev)
    h1 = sassy.DeviceReads.from_sequences([x[0] for x in d.pairs1], [x[1] for x in d.pairs1])
    h2 = sassy.DeviceReads.from_sequences([x[0] for x in d.pairs2], [x[1] for x in d.pairs2])
    s = cc.make_searcher(sassy, fx.kind)
    merged = s.merge_pairs(h1, h2, *d.pair_call)
    h1.free()
    h2.free()
    del s
    want = cc.expected("dna", "merge_pairs")[1:]
    got = cc.canon_handle(merged)
    merged.free()
    assert got == want, describe(got, want)
    # one DeviceReads (dev.reads30), a dna searcher, then an iupac one, then the dna one again
    dna, iupac = cc.make_searcher(sassy, cc.KIND["dna"]), cc.make_searcher(sassy, cc.KIND["iupac"])
    for who, s, kind_id in (("dna", dna, "dna"), ("iupac", iupac, "iupac"), ("dna again", dna, "dna")):
        for name in ("search_hamming_many_reads", "search_many_reads", "min_costs_reads"):
            check(sassy, s, fixtures(kind_id, dev), cc.by_name(name), "one DeviceReads, searcher %s" % who)


@pytest.mark.parametrize("kind_id", [k.id for k in cc.KINDS])
def test_stats_are_the_last_calls(sassy, dev, kind_id):
    """stats() after (B, A) on one searcher equals stats() of A alone on a fresh one, field by field (STATS_FIELDS).  A refused
    call is no call: it is B here, never A."""
    fx = fixtures(kind_id, dev)
    entries = [e for e in cc.entries_for(fx.kind) if not e.big]
    firsts = [e for e in entries if not e.refusal and e.name not in STATS_NOT_A_SEARCH]
    s = cc.make_searcher(sassy, fx.kind)
    wrong = []
    for i, a in enumerate(firsts):
        alone = STATS_ALONE.get((kind_id, a.name))
        if alone is None:
            fresh = cc.make_searcher(sassy, fx.kind)
            check(sassy, fresh, fx, a, (kind_id, "alone, for its stats"))
            alone = STATS_ALONE[(kind_id, a.name)] = stats_of(fresh)
        b = entries[(entries.index(a) + 11) % len(entries)]
        check(sassy, s, fx, b, (kind_id, "stats", b.name, a.name))
        check(sassy, s, fx, a, (kind_id, "stats", b.name, a.name))
        after = stats_of(s)
        diff = {f: (after[f], alone[f]) for f in STATS_FIELDS if after[f] != alone[f]}
        if diff:
            wrong.append((b.name, a.name, diff))
    assert not wrong, "kind %s: stats() after (B, A) differ from A alone, as (B, A, {field: (after, alone)}): %s" % (kind_id, wrong)
