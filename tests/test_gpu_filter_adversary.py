"""GPU: every prefilter route against the oracle on the adversary's texts (tests/helpers/filter_adversary.py): copies
with every pigeonhole piece but one destroyed, all k edits insertions or all deletions on one side of the survivor, the
counting filter's q-gram count at its threshold -- with the match ends on both sides of block, lane, wave and workgroup
borders.  A false negative of a filter drops a match without any error; here it is a missing oracle record.

Per (shape, alphabet and strand): one fresh searcher per route (options set per searcher), a first search on a short
filler text, stats() for the geometry the route really uses, the adversary for that geometry, then search and
search_all on both text lengths and once on a device-resident text at a 16-byte offset -- whole records, cigars included."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import filter_adversary as fa  # noqa: E402
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = list(fa.SHAPES)
CONFIGS = ["dna", "iupac", "iupac_ngg", "dna_rc", "iupac_rc"]
# the (filtered, fused != 0, pair != 0) a family's rows must reach on a Dna searcher, one strand: short pieces and the
# paired filter in the fused bit-plane launch, the counting filter, the bit planes fused and as the classic chain, the table
PROMISED = {
    "short": {(2, True, False)},
    "paired": {(2, True, True)},
    "counting": {(4, False, False)},
    "planes": {(2, True, False), (2, False, False)},
    "table": {(3, False, False)},
}


def key(m):
    return (m.pattern_idx, m.text_start, m.text_end, m.pattern_start, m.pattern_end, m.cost, m.strand, m.cigar)


def assert_same(got, want, ctx=None):
    """Whole records, cigars included (the convention of test_gpu_parity.py)."""
    g, w = [key(m) for m in got], [key(m) for m in want]
    if g != w:
        missing, extra = sorted(set(w) - set(g)), sorted(set(g) - set(w))
        assert False, (ctx, "missing", missing[:3], "extra", extra[:3], len(g), len(w))


class _DevText:
    """A device-resident text as the searcher takes it: data_ptr / numel / is_cuda."""

    def __init__(self, ptr, n):
        self._p, self._n = ptr, n
        self.is_cuda = True

        class _DT:
            itemsize = 1
        self.dtype = _DT()

    def data_ptr(self):
        return self._p

    def numel(self):
        return self._n

    def is_contiguous(self):
        return True


@pytest.fixture(scope="module")
def sassy():
    import sassy_amd
    assert sassy_amd.device_count() > 0, "no HIP device: the GPU tests must not silently skip"
    return sassy_amd


ROUTES = [{}] + [{"filter_kind": v} for v in (1, 2, 3, 4)] + [{"fused": 0}, {"pair": 0}, {"pair": 2}, {"short_pieces": 0},
                                                             {"count_fused": 0}, {"prefilter": 1}]


def routes(config):
    """The option rows of a configuration: the whole list on every alphabet and strand, and pair_rc where there are two strands."""
    return ROUTES + ([{"pair_rc": 0}] if config.endswith("_rc") else [])


# The rows whose route has no filter, per shape and configuration ("*": every row but prefilter = 1), as choose_route()
# (sassy_amd/csrc/scan_route.h) decides them -- replayed through tests/c/scan_route_driver.cc, the way
# tests/test_scan_route_cpu.py replays the recorded routes.  Pieces shorter than 7 rows have three filters only: the paired
# filter and the 6-row launch (both fused, bit planes) and the counting filter where it is selective.
#   - `fused` = 0 takes the two fused ones away, `pair` = 0 the paired one, `short_pieces` = 0 the 6-row launch where no pair
#     stands in, `filter_kind` 1 / 3 / 4 all of them where the counting filter is not selective (the 5-row shapes);
#   - an NGG tail lies inside the filter's rows where those reach the pattern's end (2 S Q = m or m - 2): then only
#     prefilter = 1 (the slot-mask filter, any rows) filters.
# Every other row must report filtered != 0: a route that quietly fell back to the streaming DP would still equal the oracle.
_FUSED_ONLY = "fused=0"
_PAIR_ONLY = "filter_kind=1 filter_kind=3 filter_kind=4 fused=0 pair=0"
UNFILTERED = {
    (12, 1): {"dna": _FUSED_ONLY, "iupac": _FUSED_ONLY, "dna_rc": _FUSED_ONLY, "iupac_rc": _FUSED_ONLY, "iupac_ngg": "*"},
    (18, 2): {c: "fused=0 short_pieces=0" for c in ("dna", "iupac", "dna_rc", "iupac_rc")} | {"iupac_ngg": "*"},
    (24, 3): {"dna": _FUSED_ONLY, "iupac": _FUSED_ONLY, "dna_rc": _FUSED_ONLY, "iupac_rc": _FUSED_ONLY, "iupac_ngg": "*"},
    (23, 3): {c: _PAIR_ONLY for c in CONFIGS},
    (32, 4): {c: _PAIR_ONLY for c in CONFIGS} | {"iupac_ngg": "*"},
    (32, 5): {c: _PAIR_ONLY for c in CONFIGS} | {"iupac_ngg": "*"},
    (20, 2): {"iupac_ngg": "*"},
    (27, 3): {"iupac_ngg": "filter_kind=1 filter_kind=3"},
}


def filter_expected(m, k, config, opts):
    """False exactly for the rows of UNFILTERED."""
    off = UNFILTERED.get((m, k), {}).get(config, "")
    if off == "*":
        return opts == {"prefilter": 1}
    return (",".join(f"{a}={b}" for a, b in opts.items()) or "default") not in off.split()


def pattern_of(m, k, config):
    """(pattern, its concrete copy): Iupac with an NGG tail behind the filter's rows keeps the plain pattern's own base
    under the N."""
    plain = fa.shape_pattern(m, k)
    if config == "iupac_ngg":
        return plain[:-3] + b"NGG", plain[:-3] + plain[-3:-2] + b"GG"
    return plain, plain


def make_searcher(sassy, config, opts):
    s = sassy.Searcher(config.split("_")[0], rc=config.endswith("_rc"))
    for name, value in opts.items():
        if name == "prefilter":
            s.set_prefilter(value)
        elif name == "fused":
            s.set_fused(bool(value))
        else:
            s.set_option(name, value)
    return s


def geometry_of(st, m, k):
    """The adversary's geometry for the route stats() reports."""
    if st["filtered"] == 4:
        return ("qgram", st["piece_len"])
    if st["filtered"] and st["pair"]:
        return ("pair", st["pair"], st["piece_len"])
    if st["filtered"]:
        geo = ("pieces", st["piece_len"])
        if geo not in fa.geometries(m, k) and ("qgram", st["piece_len"]) in fa.geometries(m, k):
            return ("qgram", st["piece_len"])  # both strands marked by the counting filter: stats() name the list launch behind it
        return geo
    return fa.geometries(m, k)[0]  # no filter: the widest pieces, as the streaming DP's own check


class Texts:
    """Per shape: the adversarial texts per (geometry, strands, length) and the oracle's answers, computed once."""

    def __init__(self):
        self.texts, self.answers, self.variants = {}, {}, {}

    def text(self, profile, pat, concrete, k, geo, rc, extra):
        kk = (profile, pat, geo, rc, extra)
        if kk not in self.texts:
            m = len(pat)
            kept, _ = self.screened(profile, pat, k, geo, concrete)
            flip = (lambda b: oracle.reverse_complement(profile, b)) if rc else None
            self.texts[kk] = fa.lay_out(kept, random.Random(100 * m + k), fa.MIN_BYTES, concrete, k, extra=extra, rc=flip)
        return self.texts[kk]

    def screened(self, profile, pat, k, geo, concrete):
        """(kept, dropped) of the geometry's variants through the oracle; over all of the shape's geometries at most 2 %
        of this profile's and pattern's variants may leave (the CPU test's cap, here for the Iupac patterns too)."""
        kk = (profile, pat)
        if kk not in self.variants:
            rng = random.Random(5)
            wild = {j for j, c in enumerate(pat) if c == ord("N")}
            self.variants[kk] = {g: fa.screen(oracle.search, profile, pat, k, fa.variants_for(concrete, k, g, wild), rng)
                                 for g in fa.shape_geometries(len(pat), k)}
            total = sum(len(a) + len(b) for a, b in self.variants[kk].values())
            dropped = sum(len(b) for _, b in self.variants[kk].values())
            assert dropped * 50 <= total, (profile, pat, dropped, total)
        return self.variants[kk][geo]

    def answer(self, profile, pat, text, k, rc, allm):
        kk = (profile, pat, text, k, rc, allm)
        if kk not in self.answers:
            self.answers[kk] = oracle.search(profile, pat, text, k, rc=rc, all_minima=allm)
        return self.answers[kk]


_texts = {}


def texts_of(shape):
    if shape not in _texts:
        _texts.clear()      # (one shape's texts at a time)
        _texts[shape] = Texts()
    return _texts[shape]


def planted_found(copies, want_all):
    """How many of the planted copies an oracle record overlaps."""
    ends = sorted((x.text_start, x.text_end) for x in want_all)
    found, j = 0, 0
    for c in sorted(copies, key=lambda c: c.start):
        while j < len(ends) and ends[j][1] <= c.start:
            j += 1
        found += any(a < c.end and b > c.start for a, b in ends[j:j + 64])
    return found


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"m{s[0]}k{s[1]}")
def test_filter_routes_on_adversarial_text(sassy, shape, config):
    m, k = shape
    family = fa.SHAPES[shape]
    profile, rc = config.split("_")[0], config.endswith("_rc")
    pat, concrete = pattern_of(m, k, config)
    T = texts_of(shape)
    filler = fa.filler(random.Random(7), 4096)
    seen, second_pass = set(), False
    for opts in routes(config):
        s = make_searcher(sassy, config, opts)
        assert_same(s.search(pat, filler, k), T.answer(profile, pat, filler, k, rc, False), (shape, config, opts, "filler"))
        st = s.stats()
        route = (st["filtered"], st["piece_len"], st["pair"])
        if filter_expected(m, k, config, opts):
            assert st["filtered"] != 0, (shape, config, opts, st)
        geo = geometry_of(st, m, k)
        assert geo in fa.geometries(m, k), (shape, config, opts, geo, st)
        seen.add((st["filtered"], st["fused"] != 0, st["pair"] != 0))
        # (inferred from stats(): two strands, unpaired bit planes with the full piece length and 5 .. 8 pieces are what
        # pack_filter() answers with a second launch for the Rc strand's pieces; no counter observes that launch)
        second_pass |= rc and st["filtered"] == 2 and not st["pair"] and 5 <= k + 1 <= 8 and st["piece_len"] == min(m // (k + 1), 12)
        for extra in (0, 1):
            text, copies = T.text(profile, pat, concrete, k, geo, rc, extra)
            ctx = (shape, config, opts, geo, extra, len(text))
            want, want_all = T.answer(profile, pat, text, k, rc, False), T.answer(profile, pat, text, k, rc, True)
            found = planted_found(copies, want_all)
            assert found * 100 >= 95 * len(copies), (ctx, found, len(copies))
            got = s.search(pat, text, k)
            st2 = s.stats()
            assert (st2["filtered"], st2["piece_len"], st2["pair"]) == route, (ctx, route, st2)  # the adversary's geometry
            assert_same(got, want, ctx)
            assert_same(s.search_all(pat, text, k), want_all, ctx + ("all",))
        # the same text resident on the device, 16 j bytes into an allocation that ends at the next multiple of 64 bytes
        # behind the text, counted from the text's first byte (the kernels read whole 64-byte blocks from there): exactly
        # what include/sassy_hip.h asks of a resident text, and not a byte more
        j, n = 1 + (m + k) % 3, len(text)
        buf = sassy.DeviceBuffer(16 * j + (n + 63) // 64 * 64)
        try:
            buf.upload(text, 16 * j)
            dev = _DevText(buf.ptr + 16 * j, n)
            assert_same(s.search(pat, dev, k), want, ctx + ("resident", j))
            assert_same(s.search_all(pat, dev, k), want_all, ctx + ("resident all", j))
        finally:
            buf.free()
    if config == "dna":
        assert PROMISED[family] <= seen, (shape, family, sorted(seen))
    if config == "dna_rc" and shape == (100, 5):
        assert second_pass, (shape, sorted(seen))  # 5 .. 8 pieces per strand: the Rc pieces in a launch of their own


@pytest.mark.parametrize("shape", [(20, 2), (23, 3)], ids=lambda s: f"m{s[0]}k{s[1]}")
def test_many_patterns_on_adversarial_text(sassy, shape):
    """search_encoded_patterns with the adversarial pattern among 48 of its length, on the adversarial text: the seeded
    search with its sub-piece test (seeded -1, 1), the paths without it (0), and the many-pattern bit-plane filter
    (filter_dna_multi_kernel: multi_min_text lowered to this text, neither seeded nor tiled) whose first m mod (k+1)
    pieces are a row longer -- the adversary built for those pieces.  Every pattern's records against the oracle's."""
    m, k = shape
    pat = fa.shape_pattern(m, k)
    rng = random.Random(31 * m + k)
    pats = [fa.adversary_pattern(rng, m) for _ in range(48)]
    pats[17] = pat
    rows = [{"seeded": -1, "tiled": -1}, {"seeded": 0, "tiled": -1}, {"seeded": 1, "tiled": -1}]
    if ("multi", min(m // (k + 1), 12)) in fa.shape_geometries(m, k):
        rows.append({"seeded": 0, "tiled": 0, "multi_min_text": 1})
    T = texts_of(shape)
    for opts in rows:
        geo = ("multi", min(m // (k + 1), 12)) if "multi_min_text" in opts else fa.geometries(m, k)[0]
        for extra in (0, 1):
            text, copies = T.text("dna", pat, pat, k, geo, False, extra)
            kk = ("encoded", geo, extra)
            if kk not in T.answers:
                T.answers[kk] = sorted(key(x) for x in oracle.search_encoded("dna", pats, text, k))
            want = T.answers[kk]
            mine = [w for w in want if w[0] == 17]
            assert len(mine) * 100 >= 95 * len(copies), (shape, opts, len(mine), len(copies))
            s = sassy.Searcher("dna", rc=False)
            for name, value in opts.items():
                s.set_option(name, value)
            got = s.search_encoded_patterns(s.encode_patterns(pats), text, k)
            st = s.stats()
            assert sorted(key(x) for x in got) == want, (shape, opts, extra, st["filtered"], len(got), len(want))
            if opts["seeded"] == 1:
                assert st["filtered"] == 6, (shape, opts, st)
            if "multi_min_text" in opts:
                assert st["filtered"] == 2 and st["piece_len"] == geo[1], (shape, opts, st)
