"""The batch Hamming calls restated on tests/helpers/hamming_ref.py: expected_many is hamming_ref.expected per text with the
text's index, in the contract's order; expected_best reduces those records per text by the tie order."""
import hamming_ref as href

NO_MATCH = 255
NO_PATTERN = 0xFFFFFFFF
NO_START = 0xFFFFFFFFFFFFFFFF


def expected_many(profile, patterns, texts, k, rc=False, max_n_frac=None, without_trace=False):
    """[(text_idx, oracle.Match)] of Searcher.search_hamming_many, ordered by (pattern_idx, '+' before '-', text_idx,
    text_start); the Match's coordinates are relative to its text."""
    if isinstance(patterns, (bytes, bytearray)):
        patterns = [patterns]
    rows = []
    for t, text in enumerate(texts):
        for x in href.expected(profile, patterns, bytes(text), k, rc=rc, max_n_frac=max_n_frac, without_trace=without_trace):
            rows.append((t, x))
    rows.sort(key=lambda r: (r[1].pattern_idx, 0 if r[1].strand == "+" else 1, r[0], r[1].text_start))
    return rows


def key_many(rows):
    """Comparable keys of expected_many's rows."""
    return [(t,) + href.key(x) for t, x in rows]


def key_matches(matches):
    """The same keys of the device's records (sassy_amd.Match: text_idx is a field)."""
    return [(x.text_idx,) + href.key(x) for x in matches]


def reduce_best(n_texts, rows):
    """rows: (text_idx, record) with pattern_idx / strand / text_start / cost -> per text (cost, pattern, strand 0 / 1,
    start): the smallest under (cost, pattern_idx, '+' before '-', text_start); a text without a row: the no-match tuple."""
    best = [None] * n_texts
    for t, x in rows:
        cand = (x.cost, x.pattern_idx, 0 if x.strand == "+" else 1, x.text_start)
        if best[t] is None or cand < best[t]:
            best[t] = cand
    return [(NO_MATCH, NO_PATTERN, 0, NO_START) if b is None else b for b in best]


def expected_best(profile, patterns, texts, k, rc=False, max_n_frac=None):
    """[(cost, pattern, strand, start)] per text of Searcher.hamming_best_pattern."""
    return reduce_best(len(texts), expected_many(profile, patterns, texts, k, rc=rc, max_n_frac=max_n_frac, without_trace=True))
