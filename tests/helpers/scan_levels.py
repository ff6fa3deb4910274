"""The sizes at which the device scans of hamming_pairs, fasta_unwrap and line_spans enter their upper levels, and the builders
of the inputs that the GPU tests run at those sizes.  Numpy only, no device: tests/test_scan_levels_cpu.py reads the kernels'
constants out of the sources, checks that every size below still lies beyond its threshold, and checks that every plant of
the builders sits where its comment says.

The thresholds (sassy_amd/csrc): a pairs scan block is 256 x kScanItems = 2048 rows and the top scan takes 1024 blocks per
turn; encode_list runs threaded from 65 536 sequences on; a staged tile of the pairs walk holds kPairsTileWords / (P W)
records; a FASTA or line super-tile is 16 tiles of 4 KiB and the scan over them gives each of 1024 threads `per` of them; the
FASTA record scan works in blocks of 256 x kRecPerThread = 1024 records, again 1024 threads above; the compact pass runs at
most 4096 workgroups.
"""
import functools

import numpy as np

import oracle

# ---------------------------------------------------------------- the sizes
SCAN_BLOCK = 2048                      # rows of a pairs scan block
PAIRS_BLOCK_SIZES = (2047, 2048, 2049, 4097)       # n_a, two-set mode: one block, exactly one, two, three
PAIRS_SELF_SIZES = (2049, 4097)
PAIRS_TOP_N_A = 2048 * 1024 + 2048 + 5             # 1026 scan blocks: the top scan's second turn holds blocks 1024, 1025
PAIRS_TOP_N_B = 3
ENCODE_N_B = 70001                     # targets: encode_list in 8 slices (fewer where the machine has fewer threads)
ENCODE_WORKERS = 8
SUPER = 65536                          # bytes of a super-tile (FASTA and line index)
TILE = 4096
FASTA_BIG = 1024 * SUPER + TILE + 904  # 1025 super-tiles (per = 2), 16 386 tiles (up to 5 per compact workgroup)
FASTA_MANY_RECORDS = 1048576 + 1030    # 1026 record blocks (per = 2), the last one of 6 records
REC_BLOCK = 1024
LINES_BIG = 1024 * SUPER + 4096 + 17   # 1025 super-tiles (per = 2)

# the nine instantiations of the pairs walk: (profile, P, m, W); T = 2048 / (P W) records per staged tile, U records per round
SEAM_CASES = (("dna", 2, 20, 1), ("dna", 2, 40, 2), ("dna", 2, 100, 4),
              ("iupac", 4, 20, 1), ("iupac", 4, 40, 2), ("iupac", 4, 100, 4),
              ("ascii", 8, 20, 1), ("ascii", 8, 40, 2), ("ascii", 8, 100, 4))
SEAM_K = 2


def seam_T(P, W, tile_words=2048):
    return tile_words // (P * W)


def seam_U(P, W):
    return 8 if P * W <= 4 else 32 // (P * W)


# ---------------------------------------------------------------- pairs: rows
LETTERS = {"dna": b"ACGT", "iupac": b"ACGTACGTACGTNRYKMX", "ascii": b"ACGTacgt xyzXYZ@[`{", "ascii_ci": b"ACGTacgt xyzXYZ@[`{"}


def random_rows(rng, profile, n, m):
    letters = np.frombuffer(LETTERS[profile], dtype=np.uint8)
    return letters[rng.integers(0, len(letters), size=(n, m))]


def near_copy(rng, profile, base, d):
    """base with d rows changed to another letter (under Dna and Ascii: exactly d mismatches)."""
    out = base.copy()
    letters = LETTERS[profile][:4]
    for t in rng.choice(len(base), size=min(d, len(base)), replace=False):
        out[t] = next(c for c in letters if c != base[t] and (c | 0x20) != (base[t] | 0x20))
    return out


def revcomp(profile, row):
    return np.frombuffer(oracle.reverse_complement(profile, row.tobytes()), dtype=np.uint8)


def block_borders(n):
    """the rows on both sides of every scan-block border of n rows, and the list's own ends"""
    at = {0, n - 1}
    for b in range(SCAN_BLOCK, n, SCAN_BLOCK):
        at |= {b - 1, b}
    return sorted(at)


def pairs_block_case(profile, n_a, seed, n_b=5, m=6):
    """Two-set mode over two or three scan blocks: (a, b, k).  b is random, but b[2] equals b[0] and b[1] differs from it in
    one row; about a third of a's rows are copies of a target with 0, 1 or 2 rows changed (k = 1: up to three records,
    mostly none behind two changes), the others random (nearly always an empty row); block_borders(n_a) are exact copies
    of b[0], so the rows on both sides of every block border hold records."""
    rng = np.random.default_rng(seed)
    a, b = random_rows(rng, profile, n_a, m), random_rows(rng, "dna", n_b, m)
    b[1], b[2] = near_copy(rng, "dna", b[0], 1), b[0]
    rows = np.flatnonzero(rng.random(n_a) < 0.35)
    a[rows] = b[rng.integers(0, n_b, size=len(rows))]
    changes = rng.integers(0, 3, size=len(rows))
    for t in range(2):
        hit = rows[changes > t]
        col = rng.integers(0, m, size=len(hit))
        a[hit, col] = np.where(a[hit, col] == ord("A"), ord("C"), ord("A"))
    a[block_borders(n_a)] = b[0]
    return a, b, 1


def pairs_self_case(profile, rc, n, seed, m=8):
    """Self mode over two or three scan blocks: (a, k).  Random rows at m = 8, k = 1: a row holds 0 to a few records.  Rows
    b - 1, b and b + 1 around every block border b are one sequence, so that (b - 1, b, 0) and (b, b + 1, 0) are records;
    for an rc searcher that sequence is its own reverse complement, so that (b, b, 1) is one too where b is the last row --
    without rc the last row of a triangle is empty."""
    rng = np.random.default_rng(seed)
    a = random_rows(rng, profile, n, m)
    for b in range(SCAN_BLOCK, n, SCAN_BLOCK):
        half = random_rows(rng, "dna", 1, m // 2)[0]
        a[b - 1:b + 2] = np.concatenate([half, revcomp(profile, half) if rc else half])
    return a, 1


@functools.lru_cache(maxsize=None)
def pairs_top_case():
    """(a, b, k): 2 099 205 random Dna rows of 4 bases against 3 targets, k = 1 -- about 14 % of the rows hold a record.
    block_borders(n_a), which are rows 0, 2047, 2048, ..., the last row of block 1023, the first of block 1024 and the last
    row, are copies of b[0]."""
    rng = np.random.default_rng(2048)
    a, b = random_rows(rng, "dna", PAIRS_TOP_N_A, 4), random_rows(rng, "dna", PAIRS_TOP_N_B, 4)
    a[block_borders(PAIRS_TOP_N_A)] = b[0]
    return a, b, 1


def encode_borders(n=ENCODE_N_B, workers=ENCODE_WORKERS):
    """the entries on both sides of every slice border n w / workers of encode_list, and the list's own ends"""
    at = {0, n - 1}
    for w in range(1, workers):
        at |= {n * w // workers - 1, n * w // workers}
    return sorted(at)


def encode_case(profile, seed, m=12):
    """(a, b, k) for an rc searcher: 3 entries against 70 001 random targets; the targets at encode_borders() are copies of
    a[0] with 0 .. k + 1 rows changed, every second one as its reverse complement."""
    rng = np.random.default_rng(seed)
    a, b, k = random_rows(rng, "dna", 3, m), random_rows(rng, profile, ENCODE_N_B, m), 2
    for q, j in enumerate(encode_borders()):
        b[j] = near_copy(rng, profile, a[0], q % (k + 2))
        if q % 2:
            b[j] = revcomp(profile, b[j])
    return a, b, k


# ---------------------------------------------------------------- pairs: the staged tiles of the walk
def seam_records(T, n_records):
    """the target records on both sides of the first two tile seams, and the last one"""
    return [T - 1, T, T + 1, 2 * T - 1, 2 * T, n_records - 1]


def seam_case(profile, P, m, W, rc, self_mode):
    """(a, b or None, n_records): more than 2 T + 9 target records (record r = S j + strand).  Every target j that holds one
    of seam_records() is a copy of `base` with at most k rows changed; the list of entries holds `base` and, for an rc
    searcher, its reverse complement, so that such a target is a record on strand 0 (against base) and on strand 1 (against
    the reverse complement: H(rc(base), rc(x)) = H(base, x)).  Two-set mode: 70 entries, a whole wavefront and a partial
    one.  Self mode: the targets are the entries; the first entry of every wavefront is a copy too (at most one row
    changed, as in the seam targets: any two copies lie within k = 2), so that a walk that starts inside a tile, or behind
    one, finds at least the last target."""
    S = 2 if rc else 1
    T = seam_T(P, W)
    n_t = -(-(2 * T + 10) // S)
    rng = np.random.default_rng(100 * P + W + 10 * rc + self_mode)
    base = random_rows(rng, "dna", 1, m)[0]
    other = revcomp(profile, base) if rc else near_copy(rng, profile, base, 1)
    t = random_rows(rng, profile, n_t, m)
    if self_mode:
        for q, i0 in enumerate(range(64, n_t, 64)):
            t[i0] = near_copy(rng, profile, other if rc and q % 2 else base, q % 2)
    for q, r in enumerate(seam_records(T, S * n_t)):
        t[r // S] = near_copy(rng, profile, base, q % 2)
    if self_mode:
        t[0], t[1] = base, other
        return t, None, S * n_t
    a = random_rows(rng, profile, 70, m)
    for q, i in enumerate((0, 1, 62, 63, 64, 65, 69)):
        a[i] = other if q % 2 else base
    return a, t, S * n_t


def seam_records_present(pairs, S):
    """the target records r = S b_idx + strand that the expected records hold"""
    return set((S * pairs["b_idx"].astype(np.int64) + pairs["strand"]).tolist())


def self_walk_offsets(n, S, T, chunks):
    """(i0, r_wave - rt, cnt) at the first staged tile of every (wavefront, chunk) walk of self-mode hamming_pairs -- i0 the
    wavefront's first entry, cnt the tile's records: pairs_walk and pairs_tile_first (pairs_step.h) restated -- strips of
    256 entries, wavefronts of 64, a forced chunk count."""
    chunks = max(1, min(chunks, n))
    chunk = -(-n // chunks)
    first = lambda i0, j0, j1: j0 if i0 <= j0 else min(i0, j1)  # noqa: E731
    out = []
    for c in range(-(-n // chunk)):
        j0, j1 = chunk * c, min(chunk * (c + 1), n)
        for i0 in range(0, n, 64):
            r_group, r_wave, r_end = first(i0 // 256 * 256, j0, j1) * S, first(i0, j0, j1) * S, j1 * S
            if r_wave < r_end:
                out.append((i0, r_wave - r_group, min(T, r_end - r_group)))
    return out


def self_walk_kinds(n, S, T, chunks):
    """{"at" | "inside" | "behind": [i0, ...]}: the wavefronts that start their walk at the start of their strip's first
    tile, inside it, or behind it (r_wave - rt is 0, in (0, cnt), >= cnt)"""
    kinds = {}
    for i0, off, cnt in self_walk_offsets(n, S, T, chunks):
        kinds.setdefault("at" if off == 0 else "inside" if off < cnt else "behind", []).append(i0)
    return kinds


def self_walk_chunks(n, S, T, U):
    """a forced chunk count under which some wavefront starts inside its strip's first tile at an offset that is no
    multiple of the round length U (with one chunk every offset is a multiple of 64 S).  An offset is (i0 - j0) S, a
    multiple of S, so where U <= S there is no such offset: then one that is no multiple of 64 S."""
    step = U if U > S else 64 * S
    for chunks in range(2, 40):
        if any(0 < off < cnt and off % step for _, off, cnt in self_walk_offsets(n, S, T, chunks)):
            return chunks
    raise AssertionError((n, S, T, U))


def nearest_fast(pairs, n_a):
    """hamming_pairs_ref.nearest_of_pairs without the Python loop over the records: per a_idx the first record of the
    smallest cost and how many records share that cost.  (The definition stays nearest_of_pairs: test_scan_levels_cpu.)"""
    cost = np.full(n_a, 255, dtype=np.uint8)
    index = np.full(n_a, 0xFFFFFFFF, dtype=np.uint32)
    strand = np.zeros(n_a, dtype=np.uint8)
    ties = np.zeros(n_a, dtype=np.uint32)
    if len(pairs):
        key = pairs["a_idx"].astype(np.int64) * 256 + pairs["cost"]
        order = np.argsort(key, kind="stable")  # by (a_idx, cost), the contract's order inside
        key = key[order]
        rows = key >> 8
        first = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
        best, at = pairs[order[first]], rows[first]
        cost[at], index[at], strand[at] = best["cost"], best["b_idx"], best["strand"]
        ties[at] = np.searchsorted(key, key[first], side="right") - first
    return cost, index, strand, ties


# ---------------------------------------------------------------- FASTA: 1025 super-tiles
LONG_HEADER = (509 * SUPER + 1000, 513 * SUPER + 500)  # '>' .. its '\n': begins in thread 254's pair of super-tiles (508,
#                                                        509), covers thread 255's (510, 511) whole, ends in thread 256's
FASTA_LINE = 61441                                     # bytes per sequence line, newline included


@functools.lru_cache(maxsize=None)
def _fasta_bases():
    rng = np.random.default_rng(64)
    raw = np.frombuffer(b"ACGTNacgt", dtype=np.uint8)[rng.integers(0, 9, size=FASTA_BIG, dtype=np.uint8)]
    raw[FASTA_LINE - 1::FASTA_LINE] = 10
    return raw


def fasta_big(variant):
    """64 MiB + 5000 bytes as a uint8 array, and {name: position} of what was planted.  Few records, lines of 61 440 bases.
    Byte 1024 * SUPER cannot be a '>' and the '\\n' of a CRLF at once, hence two variants:
      variant 0: '>' behind '\\n' (opens a record) as the first byte of super-tiles 2 and 1023, behind a base (opens none)
                 as the first byte of 3 and 1024;
      variant 1: '>' behind a base at 2 and 1023, behind '\\n' at 3; '\\r' is the last byte of super-tile 1023, '\\n' the
                 first of 1024, and the '>' behind it opens a record.
    Both: the long header LONG_HEADER, which also holds tile 8192 (no kept byte); eight small records inside tile 12288;
    tile 4096 and, in variant 0, tile 16384 lie inside runs of bases; the last tile, 16385, holds records that start and end
    in it.  Those are the tiles of workgroup 0 of the compact pass, in its order: 0 (a header start), 4096, 8192, 12288,
    16384."""
    raw = _fasta_bases().copy()
    at = {}

    def put(name, pos, data):
        raw[pos:pos + len(data)] = np.frombuffer(data, dtype=np.uint8)
        at[name] = pos
    put("first", 0, b">chr0 first\n")
    opens = (2, 1023) if variant == 0 else (3,)
    for s in (2, 3, 1023, 1024):
        if s in opens:
            put(f"> opens {s}", s * SUPER - 1, b"\n>s%d x\n" % s)
        elif not (variant == 1 and s == 1024):
            put(f"> in sequence {s}", s * SUPER - 1, b"A>")
    if variant == 1:
        put("crlf", 1024 * SUPER - 1, b"\r\n>behind crlf\r\nAC\r\n")
    h0, h1 = LONG_HEADER
    put("long header", h0 - 1, b"\n>")
    raw[h0 + 1:h1] = ord("h")
    raw[h0 + 7:h1:4099] = ord(">")
    raw[h0 + 9:h1:5003] = ord("\r")
    put("long header end", h1, b"\n")
    put("records in tile 12288", 12288 * TILE + 100, b"\n" + b"".join(b">t%d\nAC\r\nG\n" % i if i % 3 else b">e%d\n" % i for i in range(8)))
    put("records in the last tile", 16385 * TILE + 10, b"\n>a\nACGT\nGG\n>b\n>c d\r\nT\r\n>last\nACG")
    return raw, at


# ---------------------------------------------------------------- FASTA: 1026 record blocks
# raw bytes, id length, sequence length per kind of record; kinds 3 and 4 are the long ones at the block borders
_LONG65, _LONG4097 = b"ACGTG" * 13, b"TGCAACGTA" * 455 + b"GG"
REC_KINDS = ((b">ab\n", 2, 0), (b">a\nC\n", 1, 1), (b">\nG\r\n", 0, 1), (b">L\n" + _LONG65 + b"\n", 1, 65), (b">M\r\n" + _LONG4097 + b"\n", 1, 4097))
REC_LONG = {1023 * 1024 - 1: 3, 1023 * 1024 + 1: 4, 1024 * 1024 - 1: 4, 1024 * 1024 + 1: 3}


@functools.lru_cache(maxsize=None)
def fasta_many_records():
    """(raw bytes, {column: uint64 array}, layout bytes): 1 049 606 records of 4 to 6 raw bytes -- empty ones and one-base
    ones, mixed at random -- and, at the records REC_LONG on both sides of the borders of record blocks 1023 and 1024, one of
    65 or of 4097 bases, so that those blocks' sums differ from every other's.  The table and the layout in closed form."""
    rng = np.random.default_rng(1030)
    kinds = rng.integers(0, 3, size=FASTA_MANY_RECORDS)
    for r, kind in REC_LONG.items():
        kinds[r] = kind
    raw = b"".join([REC_KINDS[k][0] for k in kinds.tolist()])
    raw_len = np.array([len(p) for p, _, _ in REC_KINDS], dtype=np.uint64)[kinds]
    start = np.cumsum(raw_len) - raw_len
    seq_len = np.array([n for _, _, n in REC_KINDS], dtype=np.uint64)[kinds]
    slot = (seq_len + np.uint64(63)) // np.uint64(64) * np.uint64(64)
    seq_start = np.cumsum(slot) - slot
    cols = {"id_starts": start + np.uint64(1), "id_lens": np.array([n for _, n, _ in REC_KINDS], dtype=np.uint64)[kinds],
            "seq_starts": seq_start, "seq_lens": seq_len}
    layout = np.zeros(int(slot.sum()) + 64, dtype=np.uint8)
    layout[seq_start[kinds == 1].astype(np.int64)], layout[seq_start[kinds == 2].astype(np.int64)] = ord("C"), ord("G")
    for r, kind in REC_LONG.items():
        seq = _LONG65 if kind == 3 else _LONG4097
        layout[int(seq_start[r]):int(seq_start[r]) + len(seq)] = np.frombuffer(seq, dtype=np.uint8)
    return raw, cols, layout.tobytes()


def fasta_record_slices(n_rec=FASTA_MANY_RECORDS):
    """record ranges [r0, r1) on which the closed form is compared with the line-by-line parse: the first records, every
    planted border, the last (partial) block"""
    out = [(0, 2000), (n_rec - 1040, n_rec)]
    for r in (1023 * 1024, 1024 * 1024):
        out.append((r - 8, r + 8))
    return out


# ---------------------------------------------------------------- lines: 1025 super-tiles
LINES_ALL_NEWLINES = (5, 1021)  # super-tiles of 65 536 newlines


@functools.lru_cache(maxsize=None)
def lines_big():
    """64 MiB + 4096 + 17 bytes with very uneven newline counts per super-tile s: none where s % 4 is 0 or 3, one per 80
    bytes where it is 1, one per 57 where it is 2; super-tiles LINES_ALL_NEWLINES are newlines only; the last byte of
    super-tile 1023 and the first of 1024 are newlines (1023 holds no other, 1024 and the tail behind it none)."""
    a = np.full(LINES_BIG, ord("x"), dtype=np.uint8)
    body = a[:1024 * SUPER].reshape(1024, SUPER)
    body[1::4, 79::80] = 10
    body[2::4, 56::57] = 10
    for s in LINES_ALL_NEWLINES:
        body[s] = 10
    a[1024 * SUPER - 1] = a[1024 * SUPER] = 10
    return a.tobytes()


def lines_spans(n=LINES_BIG):
    """(first, last): every single position at the first and last byte of super-tiles 0, 1, 2, 3, 1022, 1023, 1024, at
    n - 1 and n; spans between neighbours of that list; spans from one scan thread's pair of super-tiles (2 t, 2 t + 1) into
    another's."""
    pos = sorted({p for s in (0, 1, 2, 3, 1022, 1023, 1024) for p in (s * SUPER, s * SUPER + SUPER - 1) if p <= n} | {n - 1, n})
    first = pos + pos[:-1]
    last = pos + pos[1:]
    for s0, s1 in ((0, 2), (1, 4), (3, 9), (4, 5), (5, 6), (6, 1020), (1019, 1022), (1021, 1024), (1023, 1024), (0, 1024)):
        first.append(s0 * SUPER + 12345)
        last.append(min(s1 * SUPER + 4321, n))
    return np.array(first, dtype=np.uint64), np.array(last, dtype=np.uint64)
