"""Searcher.hamming_counts / hamming_counts_many restated on tests/helpers/hamming_ref.py: a bincount of the expected hits'
(pattern, strand, cost) -- one text, or a list of texts summed (what hamming_many_ref's records of all texts would count to)."""
import numpy as np

import hamming_ref as href


def expected_counts(profile, patterns, text_or_texts, k, rc=False, max_n_frac=None):
    """(n_patterns, 2, k + 1) uint64: [p, strand, c] = the number of records of search_hamming (a bytes text) or of
    search_hamming_many (a list / tuple of texts) with that pattern, strand and cost.  The '-' rows stay zero without rc."""
    if isinstance(patterns, (bytes, bytearray)):
        patterns = [patterns]
    texts = [text_or_texts] if isinstance(text_or_texts, (bytes, bytearray, memoryview)) else list(text_or_texts)
    n_bins = len(patterns) * 2 * (k + 1)
    table = np.zeros(n_bins, dtype=np.uint64)
    for text in texts:
        idx, strand, _, cost = href.expected_table(profile, patterns, bytes(text), k, rc=rc, max_n_frac=max_n_frac)
        table += np.bincount((2 * idx + strand) * (k + 1) + cost, minlength=n_bins).astype(np.uint64)
    return table.reshape(len(patterns), 2, k + 1)


# A case written out by hand (tests/test_hamming_counts_cpu.py): Dna, k = 1, both strands.  ACGT is its own reverse
# complement; GG's is CC.
#   "ACGTAGGT": ACGT at 0 (0 mismatches), AGGT at 4 (1), on both strands; GG at 5 (0), "CG" 1, "GT" 2, "AG" 4, "GT" 6 (1);
#               CC: "AC" 0, "CG" 1 (1)
#   "":         nothing
#   "CC":       CC at 0 (0), the '-' strand of GG
#   "TTACGA":   ACGA at 2 (1) on both strands; GG: "CG" 3, "GA" 4 (1); CC: "AC" 2, "CG" 3 (1)
HAND_PATTERNS = [b"ACGT", b"GG"]
HAND_TEXTS = [b"ACGTAGGT", b"", b"CC", b"TTACGA"]
HAND_K = 1
HAND_PER_TEXT = [
    [[[1, 1], [1, 1]], [[1, 4], [0, 2]]],
    [[[0, 0], [0, 0]], [[0, 0], [0, 0]]],
    [[[0, 0], [0, 0]], [[0, 0], [1, 0]]],
    [[[0, 1], [0, 1]], [[0, 2], [0, 2]]],
]
HAND_TOTAL = [[[1, 2], [1, 2]], [[1, 6], [1, 4]]]
