"""What tools/record_reads_front.py records into tests/golden/reads_front.json and what tests/test_reads_front_cpu.py and
tests/test_gpu_reads_front.py replay against it: the front of the calls on a device-resident read batch -- read_overlaps,
merge_pairs, trim_reads, demux_reads, umi_groups_reads, dedup_reads, reads_slice / reads_select -- as a caller sees it.

  no_device()   code and full message of every refusal the entry points raise before a batch is read (the calls of the units'
                test_refusals_come_before_any_device_work, "everything wrong at once" included); needs no device.
  device()      the refusals that read a handle, the stats after every call and after a failed one; needs a device.

Every entry is {"call": <a name that is unique in its part>, ...}; the replay compares entry by entry."""
import ctypes as C

FAKE = 0x7000000  # a batch pointer that is never read: the refusals in front of the batch come first
STATS = ("scan_launches", "candidates", "blocks", "word_rows", "text_bytes", "filtered")


def searcher(sassy, kind):
    if kind == "overhang":
        return sassy.Searcher("iupac", rc=False, alpha=0.5)
    if kind == "only_best":
        return sassy.Searcher("dna", rc=False).only_best_match()
    if kind == "n_frac":
        return sassy.Searcher("dna", rc=False).with_max_n_frac(0.2)
    return sassy.Searcher(kind, rc=(kind == "iupac"))


def _h(reads):
    return reads._handle() if hasattr(reads, "_handle") else reads


# ---------------------------------------------------------------- the C calls: (rc, message, handle or None)
def _done(sassy, rc, handle=None):
    return int(rc), sassy.lib().sassy_hip_last_error().decode() if rc else "", handle


def c_overlaps(sassy, s, r1=FAKE, r2=FAKE, min_overlap=10, k=512, permille=200, flags=0, s_null=False, out=True):
    buf = (C.c_uint32 * (4 * 16))()
    return _done(sassy, sassy.lib().sassy_hip_read_overlaps(None if s_null else s._h, _h(r1), _h(r2), min_overlap, k, permille, flags, buf if out else None))


def c_merge(sassy, s, r1=FAKE, r2=FAKE, min_overlap=10, k=512, permille=200, flags=0, s_null=False, out=True):
    handle = C.c_void_p(7)
    rc = sassy.lib().sassy_hip_merge_pairs(None if s_null else s._h, _h(r1), _h(r2), min_overlap, k, permille, flags, None, C.byref(handle) if out else None)
    return _done(sassy, rc, handle.value if out else None)


def c_trim(sassy, s, reads=FAKE, adapters=(b"ACGTAC",), min_overlap=3, k=512, permille=100, cutoff=0, min_length=0, flags=0, s_null=False, null_at=None,
           lens=None, arrays=True, out=True):
    n = len(adapters)
    ptrs = (C.c_char_p * max(n, 1))(*[None if i == null_at else a for i, a in enumerate(adapters)])
    ls = (C.c_size_t * max(n, 1))(*(lens or [len(a) for a in adapters]))
    handle = C.c_void_p(7)
    rc = sassy.lib().sassy_hip_trim_reads(None if s_null else s._h, _h(reads), ptrs if arrays else None, ls if arrays else None, n, min_overlap, k, permille,
                                          cutoff, min_length, flags, None, C.byref(handle) if out else None)
    return _done(sassy, rc, handle.value if out else None)


def c_demux(sassy, s, reads=FAKE, barcodes=(b"ACGT", b"TTAA"), blen=None, n=None, at=0, k=1, delta=1, flags=0, s_null=False, null_at=None, array=True,
            out=True):
    nb = len(barcodes)
    ptrs = (C.c_char_p * max(nb, 1))(*[None if i == null_at else b for i, b in enumerate(barcodes)])
    handle = C.c_void_p(7)
    bounds = (C.c_uint64 * 5000)()
    rc = sassy.lib().sassy_hip_demux_reads(None if s_null else s._h, _h(reads), ptrs if array else None, len(barcodes[0]) if blen is None else blen,
                                           nb if n is None else n, at, k, delta, flags, None, None, bounds if out else None, C.byref(handle) if out else None)
    return _done(sassy, rc, handle.value if out else None)


def c_groups(sassy, s, reads=FAKE, at=0, m=12, k=1, method=2, flags=0, s_null=False, out=True):
    label = (C.c_uint32 * 16)()
    sz = C.c_size_t(0)
    rc = sassy.lib().sassy_hip_umi_groups_reads(None if s_null else s._h, _h(reads), at, m, k, method, flags, label if out else None, None, None, None,
                                                C.byref(sz), None)
    return _done(sassy, rc)


def c_dedup(sassy, s, reads=FAKE, at=0, m=12, k=1, method=2, flags=0, s_null=False, out=True):
    sz = C.c_size_t(0)
    handle = C.c_void_p(7)
    rc = sassy.lib().sassy_hip_dedup_reads(None if s_null else s._h, _h(reads), at, m, k, method, flags, None, None, None, None, None, None, C.byref(sz),
                                           C.byref(handle) if out else None)
    return _done(sassy, rc, handle.value if out else None)


def c_slice(sassy, s, reads=None, begins=None, lens=None, out=True):
    handle = C.c_void_p(7)
    return _done(sassy, sassy.lib().sassy_hip_reads_slice(_h(reads), begins, lens, None, C.byref(handle) if out else None), handle.value if out else None)


def c_select(sassy, s, reads=None, src=None, begins=None, lens=None, n_out=0, out=True):
    handle = C.c_void_p(7)
    one = (C.c_uint64 * 1)(0)
    pick = lambda a: one if a == "one" else a
    rc = sassy.lib().sassy_hip_reads_select(_h(reads), pick(src), pick(begins), pick(lens), n_out, None, C.byref(handle) if out else None)
    return _done(sassy, rc, handle.value if out else None)


ENTRY = {"read_overlaps": c_overlaps, "merge_pairs": c_merge, "trim_reads": c_trim, "demux_reads": c_demux, "umi_groups_reads": c_groups,
         "dedup_reads": c_dedup, "reads_slice": c_slice, "reads_select": c_select}


# ---------------------------------------------------------------- the calls that need no batch
def no_device_calls():
    """(entry, searcher kind, keyword arguments), in the order of the units' own tests."""
    calls = []
    add = lambda entry, kind="dna", **kw: calls.append((entry, kind, kw))
    for entry in ("read_overlaps", "merge_pairs"):
        # everything wrong at once, the faults taken away from the front one at a time
        every = dict(s_null=True, flags=1 << 20, min_overlap=0, permille=1001, r1=None, r2=None)
        add(entry, "ascii", **every)
        every.pop("s_null"); add(entry, "ascii", **every)
        every.pop("flags"); add(entry, "ascii", **every)
        every["min_overlap"] = 10; add(entry, "ascii", **every)
        every.pop("permille"); add(entry, "ascii", **every)
        add(entry, "overhang", r1=None, r2=None)
        add(entry, "only_best", r1=None, r2=None)
        add(entry, "n_frac", r1=None, r2=None)
        add(entry, "dna", r1=None, r2=None)
        # one fault at a time
        add(entry, s_null=True)
        for flags in (2, 16, 32, 1 << 20):
            add(entry, flags=flags)
        add(entry, min_overlap=0)
        add(entry, "iupac", permille=1001)
        add(entry, "iupac", permille=0xFFFFFFFF)
        for kind in ("ascii", "ascii_ci", "overhang", "only_best", "n_frac"):
            add(entry, kind)
        add(entry, r1=None)
        add(entry, r2=None)
        add(entry, "iupac", r1=None, r2=None, k=1 << 40)
    add("merge_pairs", r1=None, out=False)
    every = dict(s_null=True, flags=1, min_overlap=0, permille=1001, cutoff=94, adapters=(b"A",) * 65, reads=None)
    add("trim_reads", **every)
    every.pop("s_null"); add("trim_reads", **every)
    for flags in (2, 16, 32, 1 << 20):
        add("trim_reads", flags=flags)
    every.pop("flags"); add("trim_reads", **every)
    every["min_overlap"] = 2; add("trim_reads", "iupac", **every)
    every.pop("permille"); add("trim_reads", **every)
    every.pop("cutoff"); add("trim_reads", **every)
    add("trim_reads", "ascii", arrays=False, reads=None)
    add("trim_reads", "ascii", adapters=(b"ACGT", b"ACGT"), null_at=1, reads=None)
    add("trim_reads", "ascii", adapters=(b"ACGT", b"ACGT"), lens=[4, 0], reads=None)
    add("trim_reads", "ascii", adapters=(b"A" * 65,), reads=None)
    add("trim_reads", "ascii", adapters=(b"ACGT", b"ACGTA", b"ACG"), min_overlap=4, reads=None)
    for kind in ("ascii", "ascii_ci", "overhang", "only_best", "n_frac", "dna"):
        add("trim_reads", kind, reads=None)
    add("trim_reads", reads=None, adapters=())
    add("trim_reads", reads=None, out=False)
    every = dict(s_null=True, flags=4, delta=66, n=0, blen=0, array=False, at=600, reads=None)
    add("demux_reads", **every)
    every.pop("s_null"); add("demux_reads", **every)
    for flags in (4 | 3, 4, 1 << 20, 32 << 8 | 1):
        add("demux_reads", flags=flags)
    every.pop("flags"); add("demux_reads", "iupac", **every)
    every.pop("delta"); add("demux_reads", **every)
    every["n"] = 4097; add("demux_reads", **every)
    every.pop("n"); add("demux_reads", **every)
    every["blen"] = 65; add("demux_reads", **every)
    every.pop("blen"); add("demux_reads", "ascii", **every)
    every.pop("array"); add("demux_reads", "ascii", null_at=1, **every)
    add("demux_reads", "ascii", **every)
    add("demux_reads", "ascii", at=509, reads=None)
    for kind in ("ascii", "ascii_ci"):
        add("demux_reads", kind, at=508, reads=None)
    for kind in ("overhang", "only_best", "n_frac", "dna"):
        add("demux_reads", kind, reads=None)
    add("demux_reads", reads=None, flags=3, delta=0, k=1 << 40)
    add("demux_reads", reads=None, out=False)
    for entry in ("umi_groups_reads", "dedup_reads"):
        every = dict(s_null=True, flags=2, method=3, m=0, at=600, reads=None, out=False)
        add(entry, "ascii", **every)
        every.pop("s_null"); add(entry, "ascii", **every)
        for flags in (2 | 1, 2, 1 << 20, 32 << 8 | 1):
            add(entry, flags=flags)
        every.pop("flags"); add(entry, "ascii", **every)
        every.pop("method"); add(entry, "ascii", **every)
        every["m"] = 129; add(entry, "ascii", **every)
        every["m"] = 12; add(entry, "ascii", **every)
        add(entry, "ascii", at=385, m=128, reads=None, out=False)
        for kind in ("ascii", "ascii_ci"):
            add(entry, kind, at=384, m=128, reads=None, out=False)
        for kind in ("overhang", "only_best", "n_frac", "dna"):
            add(entry, kind, reads=None, out=False)
        add(entry, "iupac", reads=None, flags=1, k=1 << 40, method=0, m=128, at=384)
    add("reads_slice")
    add("reads_slice", reads=FAKE, out=False)
    add("reads_select")
    add("reads_select", reads=FAKE, n_out=3)
    add("reads_select", reads=FAKE, src="one", begins="one")
    add("reads_select", reads=FAKE, src="one", lens="one")
    add("reads_select", reads=FAKE, src="one", n_out=1 << 32)
    return calls


def _name(i, entry, kind, kw):
    return "%03d %s %s %s" % (i, entry, kind, " ".join("%s=%s" % (k, len(v) if isinstance(v, tuple) else v) for k, v in sorted(kw.items())))


def no_device(sassy):
    made = {}
    entries = []
    for i, (entry, kind, kw) in enumerate(no_device_calls()):
        s = made.setdefault(kind, searcher(sassy, kind))
        rc, msg, handle = ENTRY[entry](sassy, s, **kw)
        assert rc != 0 and handle is None, (entry, kind, kw, rc, handle)   # a refusal, and it hands nothing out
        entries.append({"call": _name(i, entry, kind, kw), "rc": rc, "msg": msg})
    return entries


# ---------------------------------------------------------------- the calls that read a batch
def _stats(s):
    st = s.stats()
    return {k: int(st[k]) for k in STATS}


def batches(sassy):
    """The read batches of the device part, by name; every read of the stats' batches has at most 40 bytes."""
    q = lambda seqs: [bytes(33 + (7 * i + j) % 40 for j in range(len(x))) for i, x in enumerate(seqs)]
    R = sassy.DeviceReads.from_sequences
    five = [b"ACGTACGTTTGACCAGTAGGCATAGATCGGAAG", b"TTGACCAGTAACGTACGTAGGCATAG", b"ACG", b"ACGTACGTTTGACCAGTAGGCATAGATCGGAAGAGCACA", b"GGGTTTCCCAAATTTGGGCCCAAA"]
    mates = [b"CTTCCGATCTATGCCTACTGGTCAAACGTACGT", b"CTATGCCTACGTACGTTACTGGTCAA", b"CGT", b"TGTGCTCTTCCGATCTATGCCTACTGGTCAAACGTACGT", b"AAACCCGGGTTTAAACCCGGG"]
    with_n = list(five)
    with_n[1] = b"TTGACCAGTAACGNACGTAGGCATAG"
    out = {
        "short": R([b"ACGT", b"ACG"]), "short_q": R([b"ACGT", b"ACG"], q([b"ACGT", b"ACG"])), "three": R([b"ACGT", b"ACG", b"A"]),
        "long": R([b"ACGT", b"A" * 513]), "long_q": R([b"ACGT", b"A" * 513], q([b"ACGT", b"A" * 513])),
        "b0": R([], []), "m0": R([], []),
        "b1": R(five[:1], q(five[:1])), "m1": R(mates[:1], q(mates[:1])),
        "b5": R(five, q(five)), "m5": R(mates, q(mates)),
        "n5": R(with_n, q(with_n)),
    }
    return out


def same_batch(a, b):
    """Two handles hold the same batch, byte for byte: the table, the text, the per-block table, the qualities."""
    import numpy as np
    ok = len(a) == len(b) and a.text_bytes == b.text_bytes and a.longest == b.longest and bool(a.qual_ptr) == bool(b.qual_ptr)
    ok = ok and np.array_equal(a.seq_starts, b.seq_starts) and np.array_equal(a.seq_lens, b.seq_lens)
    ok = ok and a.download_text() == b.download_text() and np.array_equal(a.download_rem(), b.download_rem())
    return bool(ok and (not a.qual_ptr or a.download_quality_text() == b.download_quality_text()))


def device(sassy):
    """{"refusals": [...], "stats": [...]}: see the module's doc.  `same` of a stats entry: the batch the call returned equals
    the windows of its source that reads_slice / reads_select make (a merge: the identity slice of the merged batch)."""
    import numpy as np
    B = batches(sassy)
    refusals, stats = [], []

    def refused(name, entry, s, **kw):
        rc, msg, handle = ENTRY[entry](sassy, s, **kw)
        assert rc != 0 and handle is None, (name, rc, handle)
        refusals.append({"call": name, "rc": rc, "msg": msg, "stats": _stats(s)})

    one = {"read_overlaps": lambda r: dict(r1=r, r2=r), "merge_pairs": lambda r: dict(r1=r, r2=r)}
    six = ("read_overlaps", "merge_pairs", "trim_reads", "demux_reads", "umi_groups_reads", "dedup_reads")
    args = lambda entry, r: one.get(entry, lambda r: dict(reads=r))(r)
    for kind in ("dna", "iupac"):
        s = searcher(sassy, kind)
        for entry in six:
            refused("%s %s too long" % (kind, entry), entry, s, **args(entry, B["long_q"]))
            refused("%s %s too long, no out" % (kind, entry), entry, s, out=False, **args(entry, B["long_q"]))
            refused("%s %s no out" % (kind, entry), entry, s, out=False, **args(entry, B["short_q"]))
        refused(kind + " read_overlaps too long first", "read_overlaps", s, r1=B["long"], r2=B["short"])
        refused(kind + " read_overlaps too long second", "read_overlaps", s, r1=B["short"], r2=B["long"])
        refused(kind + " read_overlaps counts", "read_overlaps", s, r1=B["short"], r2=B["three"])
        refused(kind + " merge_pairs counts", "merge_pairs", s, r1=B["short_q"], r2=B["three"])
        refused(kind + " merge_pairs counts before too long", "merge_pairs", s, r1=B["long_q"], r2=B["three"])
        refused(kind + " merge_pairs no quality first", "merge_pairs", s, r1=B["short"], r2=B["short_q"])
        refused(kind + " merge_pairs no quality second", "merge_pairs", s, r1=B["short_q"], r2=B["short"])
        refused(kind + " merge_pairs too long before no quality", "merge_pairs", s, r1=B["long"], r2=B["long"])
        refused(kind + " merge_pairs no quality before no out", "merge_pairs", s, r1=B["short"], r2=B["short"], out=False)
        refused(kind + " trim_reads no quality", "trim_reads", s, reads=B["short"], cutoff=20)
        refused(kind + " trim_reads too long before no quality", "trim_reads", s, reads=B["long"], cutoff=20)
        refused(kind + " trim_reads no quality before no out", "trim_reads", s, reads=B["short"], cutoff=20, out=False)
    # searches in flight: a ticket is open on the searcher
    s = searcher(sassy, "dna")
    text = sassy.DeviceBuffer(256 + 256)
    text.upload(b"ACGT" * 64)
    ticket = s.search_shard_begin(b"ACGTACGTACGT", text.ptr, 0, 256, 0, 256, 1)
    for entry in six:
        refused("in flight %s" % entry, entry, s, **args(entry, B["short_q"]))
        refused("in flight %s too long" % entry, entry, s, **args(entry, B["long_q"]))
        refused("in flight %s no out" % entry, entry, s, out=False, **args(entry, B["short_q"]))
    s.search_finish(ticket)
    text.free()
    # another device than the searcher's: only where there are two
    if sassy.device_count() >= 2:
        s = searcher(sassy, "dna")
        s.set_device(1)
        for entry in six:
            refused("other device %s" % entry, entry, s, **args(entry, B["short_q"]))
            refused("other device %s too long" % entry, entry, s, **args(entry, B["long_q"]))

    # ---- the stats after every call, and what the call returned
    def ran(name, s, fn, check):
        try:
            got = fn()
        except sassy.SassyHipError as e:
            stats.append({"call": name, "error": str(e), "stats": _stats(s)})
            return
        entry = {"call": name, "stats": _stats(s)}
        if check is not None:
            entry["same"] = check(got)
            entry["stats_after_windows"] = _stats(s)   # the window calls have no searcher: its stats stay
        stats.append(entry)

    def demux_same(reads):
        def check(d):
            m, at = 4, 2
            assigned = d.records["sample"][d.order.astype(np.int64)] >= 0 if len(d.order) else np.zeros(0, dtype=bool)
            return same_batch(d.reads, reads.select(d.order, np.where(assigned, at + m, 0), d.reads.seq_lens))
        return check

    for kind in ("dna", "iupac"):
        for size in ("0", "1", "5"):
            s = searcher(sassy, kind)
            b, m = B["b" + size], B["m" + size]
            tag = "%s n=%s " % (kind, size)
            ran(tag + "read_overlaps", s, lambda: s.read_overlaps(b, m, min_overlap=8), None)
            ran(tag + "merge_pairs", s, lambda: s.merge_pairs(b, m, min_overlap=8), lambda g: same_batch(g, g.slice(0, g.seq_lens)))
            ran(tag + "trim_reads", s, lambda: s.trim_reads(b, [b"AGATCGGAAG", b"GGCATAG"], min_overlap=5, quality_cutoff=20, with_records=True),
                lambda g: same_batch(g[0], b.slice(0, g[1]["length"].astype(np.uint64))))
            ran(tag + "demux_reads", s, lambda: b.demux(s, [b"GTAC", b"GACC", b"GTTT"], k=1, at=2, with_records=True), demux_same(b))
            ran(tag + "umi_groups_reads", s, lambda: b.umi_groups(s, 8, k=1), None)
            ran(tag + "dedup_reads", s, lambda: b.dedup(s, 8, k=1), lambda g: same_batch(g.reads, b.select(g.kept)))
            ran(tag + "dedup_reads no window", s, lambda: b.dedup(s, 41, k=1), lambda g: same_batch(g.reads, b.select(g.kept)))
            ran(tag + "reads_slice", s, lambda: b.slice(1, np.maximum(b.seq_lens, 1) - 1), lambda g: same_batch(g, b.select(np.arange(len(b)), 1, g.seq_lens)))
            ran(tag + "reads_select", s, lambda: b.select(np.arange(len(b))[::-1]), lambda g: same_batch(g.select(np.arange(len(b))[::-1]), b))
        # a batch that holds an N: a dna searcher refuses it after the look, an iupac searcher runs it
        s = searcher(sassy, kind)
        b, m = B["n5"], B["m5"]
        tag = "%s N " % kind
        ran(tag + "read_overlaps", s, lambda: s.read_overlaps(b, m, min_overlap=8), None)
        ran(tag + "read_overlaps second", s, lambda: s.read_overlaps(m, b, min_overlap=8), None)
        ran(tag + "merge_pairs", s, lambda: s.merge_pairs(b, m, min_overlap=8), None)
        ran(tag + "trim_reads", s, lambda: s.trim_reads(b, [b"AGATCGGAAG"], min_overlap=5), None)
        ran(tag + "trim_reads adapter", s, lambda: s.trim_reads(b, [b"AGATCGGNAG"], min_overlap=5), None)
        ran(tag + "demux_reads", s, lambda: b.demux(s, [b"GTAC", b"GACC"], at=2), None)
        ran(tag + "demux_reads barcode", s, lambda: b.demux(s, [b"GTAC", b"GNCC"], at=2), None)
        ran(tag + "umi_groups_reads", s, lambda: b.umi_groups(s, 8), None)
        ran(tag + "dedup_reads", s, lambda: b.dedup(s, 8), None)
        ran(tag + "dedup_reads no window", s, lambda: b.dedup(s, 41), None)
    for r in B.values():
        r.free()
    return {"refusals": refusals, "stats": stats}
