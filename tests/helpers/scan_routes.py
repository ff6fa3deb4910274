"""Shared by tools/record_scan_routes.py (which writes tests/golden/scan_routes.json), tests/test_gpu_routes.py (which
replays it on a device) and tests/test_scan_route_cpu.py (which replays it through csrc/scan_route.h on the host): the
sweep's texts, its rows, and how a row is run.  A row is
  {"alphabet", "rc", "alpha" (null: none), "pattern" (classes: the expression), "k", "opts": {...}, "classes" (optional)}
and its recorded "stats" = [filtered, piece_len, fused, pair, number of matches]."""
import random

import prose_text

TEXT_BYTES = 1 << 16
PLANT_AT = 30011
BYTE_MODE_PATTERN = bytes(range(33, 127))  # 94 distinct bytes (52 + 42 folded): more than the 64 mask slots

# (m, k): short pieces | 5-row pieces | paired | count filter | planes, table, several words | pieces too short
SHAPES = [(12, 1), (18, 2), (24, 3), (11, 1), (15, 2), (23, 3), (32, 4), (32, 5), (20, 2), (27, 3),
          (32, 3), (40, 2), (64, 3), (65, 3), (100, 5), (300, 8), (32, 12)]
# Every row costs a fresh searcher (about 20 ms with its first search), so an option runs over the shapes it bears on:
SHORT, PAIRED, COUNTED = [(12, 1), (18, 2), (24, 3)], [(23, 3), (32, 4), (32, 5)], [(20, 2), (27, 3)]
ONE_OF_EACH = [(12, 1), (23, 3), (20, 2), (32, 3), (64, 3)]
RC_SHAPES = [(12, 1), (23, 3), (32, 4), (20, 2), (32, 3), (64, 3), (100, 5), (32, 12)]
KIND_SHAPES = [(24, 3), (23, 3), (20, 2), (32, 3), (64, 3), (100, 5), (300, 8)]

_FIRST_BASE = {"R": "A", "Y": "C", "K": "G", "M": "A", "S": "C", "W": "A", "N": "T", "B": "C", "D": "A", "H": "A", "V": "A"}


def dna_pattern(m, k, kind):
    """kind: 'plain' | 'ngg' (plain prefix, NGG tail) | 'ambig' (an ambiguity letter every third row)."""
    rng = random.Random(1000 * m + k)
    p = [rng.choice("ACGT") for _ in range(m)]
    if kind == "ngg" and m >= 3:
        p[-3:] = "NGG"
    if kind == "ambig":
        for j in range(1, m, 3):
            p[j] = "RYKMSWN"[(j // 3) % 7]
    return "".join(p)


def concrete(pattern):
    return "".join(_FIRST_BASE.get(c, c) for c in pattern)


def texts():
    """{'dna': bytes, 'prose': bytes}: the two seeded 64 KiB texts without plants."""
    rng = random.Random(20260)
    dna = bytes(rng.choice(b"ACGT") for _ in range(TEXT_BYTES))
    return {"dna": dna, "prose": prose_text.prose(random.Random(20261), TEXT_BYTES)}


def row_text(base, row):
    """The row's text: the seeded text with the pattern planted once (prose patterns are cut from the text itself)."""
    if row["alphabet"] in ("dna", "iupac"):
        t = bytearray(base["dna"])
        p = concrete(row["pattern"]).encode()
        t[PLANT_AT:PLANT_AT + len(p)] = p
        return bytes(t)
    if row.get("classes"):
        return base["prose"]
    t = bytearray(base["prose"])
    p = row["pattern"].encode("latin-1")
    t[PLANT_AT:PLANT_AT + len(p)] = p
    return bytes(t)


def rows(prose):
    out = []

    def add(alphabet, rc, pattern, k, opts=None, alpha=None, classes=False):
        r = {"alphabet": alphabet, "rc": rc, "alpha": alpha, "pattern": pattern, "k": k, "opts": dict(opts or {})}
        if classes:
            r["classes"] = True
        out.append(r)

    DNA, PLAIN, NGG, AMBIG = ("dna", "plain"), ("iupac", "plain"), ("iupac", "ngg"), ("iupac", "ambig")

    def sweep(kinds, shapes, opts, rc=False, alpha=None):
        for alphabet, kind in kinds:
            for m, k in shapes:
                add(alphabet, rc, dna_pattern(m, k, kind), k, opts, alpha)

    # every shape, every pattern kind, one strand; both strands for Dna and plain Iupac, elsewhere the shapes that differ
    sweep([DNA, PLAIN, NGG, AMBIG], SHAPES, {})
    sweep([DNA, PLAIN], SHAPES, {}, rc=True)
    sweep([NGG, AMBIG], RC_SHAPES, {}, rc=True)
    sweep([PLAIN, NGG, AMBIG], [(32, 3)], {}, alpha=0.5)  # (iupac: the only alphabet whose searcher takes an overhang)
    sweep([PLAIN], [(24, 3), (23, 3), (20, 2)], {}, alpha=0.5)
    sweep([PLAIN], [(32, 3)], {}, rc=True, alpha=0.5)
    for v in (0, 1):
        sweep([DNA], SHAPES, {"prefilter": v})
        sweep([AMBIG], ONE_OF_EACH, {"prefilter": v})
    for v in (0, 2):
        sweep([DNA, NGG], SHORT + PAIRED + COUNTED, {"pair": v})
    for v in (1, 2, 3, 4):
        sweep([DNA], KIND_SHAPES, {"filter_kind": v})
        sweep([AMBIG], KIND_SHAPES[:4], {"filter_kind": v})
    sweep([DNA, PLAIN], SHORT, {"short_pieces": 0})
    sweep([PLAIN, NGG], [(12, 1), (24, 3), (23, 3), (32, 4), (32, 3), (64, 3)], {"iupac_planes": 0})
    sweep([DNA, PLAIN, NGG, AMBIG], COUNTED, {"count_fused": 0})
    for name in ("trace_wave", "self_rank", "fused", "trace"):
        sweep([DNA, PLAIN], ONE_OF_EACH, {name: 0})
    for name, value in [("prefilter", 0), ("prefilter", 1), ("pair", 0), ("filter_kind", 1), ("filter_kind", 2), ("filter_kind", 3),
                        ("filter_kind", 4), ("count_fused", 0), ("fused", 0), ("pair_rc", 0)]:
        sweep([DNA], [(23, 3), (20, 2), (100, 5)], {name: value}, rc=True)
    sweep([PLAIN], [(23, 3), (32, 3)], {"pair_rc": 0}, rc=True)
    sweep([PLAIN], [(20, 2), (32, 3)], {"filter_kind": 4}, rc=True)
    # a second option next to the one that changes what it bears on
    for opts in ({"pair": 2, "count_fused": 0}, {"pair": 0, "short_pieces": 0}, {"fused": 0, "filter_kind": 2}, {"prefilter": 1, "filter_kind": 1}):
        sweep([DNA, NGG], [(23, 3), (20, 2), (24, 3)], opts)
    # Ascii: patterns cut from the prose -- few distinct bytes, more than 16, byte mode
    cuts = [(5000, 12, 1), (5000, 24, 3), (7000, 16, 1), (9000, 40, 2), (9000, 64, 3), (12000, 100, 5), (12000, 32, 12)]
    for alphabet in ("ascii", "ascii_ci"):
        for at, m, k in cuts:
            p = prose[at:at + m].decode("latin-1")
            for opts in ({}, {"prefilter": 0}, {"prefilter": 1}, {"filter_kind": 1}) if m in (12, 40, 64) else ({},):
                add(alphabet, False, p, k, opts)
        for opts in ({}, {"prefilter": 1}):
            add(alphabet, False, BYTE_MODE_PATTERN.decode("latin-1"), 4, opts)
        add(alphabet, False, "[Tt]imeout[ ,._]", 1, classes=True)
    return out


def run_row(sassy, base, row):
    """One search on a fresh searcher (the lane's table cache and fuse back-off in their initial state): the row's stats."""
    s = sassy.Searcher(row["alphabet"], rc=row["rc"], alpha=row["alpha"])
    trace = True
    for name, value in row["opts"].items():
        if name == "prefilter":
            s.set_prefilter(value)
        elif name == "fused":
            s.set_fused(bool(value))
        elif name == "trace":
            trace = bool(value)
        else:
            s.set_option(name, value)
    text = row_text(base, row)
    if row.get("classes"):
        got = s.search_classes(row["pattern"].encode("latin-1"), text, row["k"])
    elif trace:
        got = s.search(row["pattern"].encode("latin-1"), text, row["k"])
    else:
        got = s.search_without_trace(row["pattern"].encode("latin-1"), text, row["k"])
    st = s.stats()
    return [st["filtered"], st["piece_len"], st["fused"], st["pair"], len(got)]
