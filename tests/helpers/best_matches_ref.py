"""The expected result of Searcher.best_matches from the CPU oracle's matches, by the definition in include/sassy_hip.h:
of the records search_many gives for a text (only_best_match off) the one that is smallest under

    1. lowest cost;  2. lowest pattern_idx;  3. Fwd before Rc;
    4. the rightmost end in the strand's scan direction: the largest text_end for Fwd, the smallest text_start for Rc
       (the Rc strand is scanned on the reversed text; reference: src/search.rs:1392-1412, "rightmost match with minimal
       cost"); of two overhang matches that end behind the text's end the one that hangs over further -- the smaller
       pattern_end -- ends further right.

Works on anything with the Match attributes (oracle.Match, sassy_amd.Match, raw _OrcMatch rows): strand '+' / '-' or 0 / 1."""
from concurrent.futures import ThreadPoolExecutor

import oracle


def is_rc(m) -> int:
    return 1 if m.strand in ("-", 1) else 0


def order_key(m, pattern_idx=None):
    rc = is_rc(m)
    return (m.cost, m.pattern_idx if pattern_idx is None else pattern_idx, rc, m.text_start if rc else -m.text_end, m.pattern_end)


def best_of(matches):
    """The best of one text's matches (each carries its pattern_idx), None if there are none."""
    matches = list(matches)
    return min(matches, key=order_key) if matches else None


def record(m, text_idx, pattern_idx=None):
    """The fields best_matches' records are compared by."""
    return (text_idx, m.pattern_idx if pattern_idx is None else pattern_idx, m.text_start, m.text_end, m.pattern_start, m.pattern_end,
            m.cost, "-" if is_rc(m) else "+", m.cigar)


def got_record(m):
    return record(m, m.text_idx)


def expected(search, patterns, texts):
    """search(pattern, text) -> the oracle's matches of one pair.  The records of the expected result, ascending text_idx."""
    out = []
    for ti, t in enumerate(texts):
        best = None
        for pi, p in enumerate(patterns):
            for m in search(p, t):
                key = order_key(m, pi)
                if best is None or key < best[0]:
                    best = (key, record(m, ti, pi))
        if best is not None:
            out.append(best[1])
    return out


def expected_fast(profile, patterns, texts, k, rc, threads=16):
    """The same for a read set (10^6 pairs) through the oracle's C entry point: a Python object only for each text's winner;
    the texts are shared out over threads (the oracle call releases the GIL)."""
    L = oracle.lib()
    prof = oracle._profile(profile)
    import ctypes as C

    def one(ti):
        t = texts[ti]
        best = None
        for pi, p in enumerate(patterns):
            res = L.orc_search(prof, int(rc), 0, p, len(p), t, len(t), k)
            try:
                n = L.orc_result_len(res)
                if n == 0:
                    continue
                assert not L.orc_result_failed(res)
                ms = L.orc_result_matches(res)
                ops_ptr = L.orc_result_ops(res)
                for i in range(n):
                    m = ms[i]
                    key = (m.cost, pi, 1 if m.strand else 0, m.text_start if m.strand else -m.text_end, m.pattern_end)
                    if best is None or key < best[0]:
                        ops = C.string_at(ops_ptr + m.cigar_off, m.cigar_len) if m.cigar_len else b""
                        best = (key, (ti, pi, m.text_start, m.text_end, m.pattern_start, m.pattern_end, m.cost,
                                      "-" if m.strand else "+", oracle.rle_cigar(ops)))
            finally:
                L.orc_result_free(res)
        return best[1] if best else None

    with ThreadPoolExecutor(threads) as ex:
        return [r for r in ex.map(one, range(len(texts))) if r is not None]


def without_trace(rec):
    """What a record carries when searched without trace (src/search.rs:1464-1475, 859-873): the end in scan direction and
    the cost; no start, no cigar."""
    NONE = (1 << 64) - 1
    ti, pi, ts, te, ps, pe, cost, strand, _ = rec
    return (ti, pi, ts if strand == "-" else NONE, NONE if strand == "-" else te, NONE, pe, cost, strand, "")
