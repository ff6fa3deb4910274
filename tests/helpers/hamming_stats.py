"""Shared by tools/record_hamming_stats.py (which writes tests/golden/hamming_stats.json) and tests/test_gpu_hamming_stats.py
(which replays it on a device): the calls of the Hamming family whose stats() are pinned, and how a call is run.  A call is
  {"entry", "alphabet", "rc", "k", "patterns": [indices into the text set's patterns or pairs], "opts": {...}}
(the batch entry points take batch(text), the others the whole text) and its recorded "stats" = the whole stats() dict without the *_ms fields, plus "records": what the call returned, counted."""
import random

TILE_BYTES = 4096
TEXT_BYTES = 3 * TILE_BYTES + 100  # three tiles and a partial one
ROWS = (1, 64, 65, 130)            # halo blocks 0, 1, 1 and 3
BATCH_LENS = (4000, 0, 4100)
FORCED = {"hamming_items": 64, "hamming_records": 7, "hamming_batch": 1}
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(p):
    return bytes(p).translate(_COMP)[::-1]


def texts():
    """{'dna', 'ascii': the two seeded texts; 'patterns': the Dna patterns of ROWS rows; 'ascii_patterns': two patterns of
    disjoint 40-byte alphabets; 'pairs': two primer pairs} -- every pattern is planted, the long ones once exact and once
    with two substitutions, across tile borders too."""
    rng = random.Random(20261019)
    dna = bytearray(rng.choice(b"ACGT") for _ in range(TEXT_BYTES))
    patterns = [bytes(rng.choice(b"ACGT") for _ in range(m)) for m in ROWS]
    for i, p in enumerate(patterns[1:]):
        # across the border of tiles i and i + 1; with two substitutions; for the 64 rows, at the text's very end
        for at, subs in ((TILE_BYTES * (i + 1) - 17 - 20 * i, 0), (700 + 2500 * i, 2), (TEXT_BYTES - 64, 0))[:3 if i == 0 else 2]:
            q = bytearray(p)
            for j in range(subs):
                q[5 + 9 * j] = ord("A") if q[5 + 9 * j] != ord("A") else ord("C")
            dna[at:at + len(q)] = q
            if i == 0 and at + 200 + len(q) <= TEXT_BYTES:  # the minus strand of an rc searcher
                dna[at + 200:at + 200 + len(q)] = revcomp(q)
    pairs = [(bytes(rng.choice(b"ACGT") for _ in range(20)), bytes(rng.choice(b"ACGT") for _ in range(22))) for _ in range(2)]
    for i, (f, r) in enumerate(pairs):
        for at, length in ((1000 + 5000 * i, 300), (TILE_BYTES + 3000 + 300 * i, 1200)):
            dna[at:at + len(f)] = f
            dna[at + length - len(r):at + length] = revcomp(r)
        at = 9000 + 1500 * i  # strand 1: rev in front, the reverse complement of fwd behind
        dna[at:at + len(r)] = r
        dna[at + 400 - len(f):at + 400] = revcomp(f)
    alpha = [bytes(range(33, 73)), bytes(range(73, 113))]
    asc = bytearray(rng.choice(alpha[0] + alpha[1]) for _ in range(TEXT_BYTES))
    ascii_patterns = [bytes(rng.sample(list(a), 40)) for a in alpha]
    for i, p in enumerate(ascii_patterns):
        asc[TILE_BYTES * (i + 1) - 11:TILE_BYTES * (i + 1) - 11 + 40] = p
        asc[300 + 5000 * i:300 + 5000 * i + 40] = p[:20] + bytes([p[21], p[20]]) + p[22:]
    assert len(dna) == len(asc) == TEXT_BYTES
    return {"dna": bytes(dna), "ascii": bytes(asc), "patterns": patterns, "ascii_patterns": ascii_patterns, "pairs": pairs}


def batch(text):
    out, at = [], 0
    for n in BATCH_LENS:
        out.append(text[at:at + n])
        at += n
    return out


def calls():
    out = []
    for entry in ("search_hamming", "hamming_counts", "search_hamming_many", "hamming_best_pattern", "hamming_counts_many", "hamming_amplicons"):
        many = entry in ("search_hamming_many", "hamming_best_pattern", "hamming_counts_many")
        option_sets = [{}, dict(FORCED)]
        if many:
            option_sets += [{"hamming_many_batch": 8192}, dict(FORCED, hamming_many_batch=8192), {"hamming_many_batch": 4096}]
        for opts in option_sets:
            for rc in (False, True):
                for k in (0, 2):
                    if entry == "hamming_amplicons":
                        out.append({"entry": entry, "alphabet": "dna", "rc": rc, "k": k, "patterns": [0, 1], "opts": opts})
                        continue
                    lists = [[0, 1, 2, 3]] + ([[0], [1], [2], [3]] if entry in ("search_hamming", "hamming_counts") else [])
                    for which in lists:
                        out.append({"entry": entry, "alphabet": "dna", "rc": rc, "k": k, "patterns": which, "opts": opts})
            if entry != "hamming_amplicons":  # two groups: the patterns share no slot
                out.append({"entry": entry, "alphabet": "ascii", "rc": False, "k": 2, "patterns": [0, 1], "opts": opts})
    return out


def run_call(sassy, base, call):
    """One call on a fresh searcher: its stats() without the times, and the number of records (counts: their sum)."""
    s = sassy.Searcher(call["alphabet"], rc=call["rc"])
    for name, value in call["opts"].items():
        s.set_option(name, value)
    ascii_ = call["alphabet"] == "ascii"
    text = base["ascii" if ascii_ else "dna"]
    pats = [base["ascii_patterns" if ascii_ else "patterns"][i] for i in call["patterns"]]
    entry, k = call["entry"], call["k"]
    if entry == "search_hamming":
        records = len(s.search_hamming(pats, text, k))
    elif entry == "hamming_counts":
        records = int(s.hamming_counts(pats, text, k).sum())
    elif entry == "search_hamming_many":
        records = len(s.search_hamming_many(pats, batch(text), k))
    elif entry == "hamming_best_pattern":
        records = int((s.hamming_best_pattern(pats, batch(text), k)[0] != 255).sum())
    elif entry == "hamming_counts_many":
        records = int(s.hamming_counts_many(pats, batch(text), k).sum())
    else:
        records = len(s.hamming_amplicons([base["pairs"][i] for i in call["patterns"]], text, k, 50, 5000))
    st = {name: value for name, value in s.stats().items() if not name.endswith("_ms")}
    st["records"] = records
    return st
