"""`python -m sassy_amd search | filter | demux | count | amplicon | pairs | cluster ...` -- the match-table and the record-filter front ends of the reference CLI on the GPU path.

Mirrors `sassy search` (reference: bin/grep.rs:30-157 arguments, :465-470 header, :623-660 pattern
sources, :710-757 rows; FASTA/FASTQ records as bin/input_iterator.rs:125-137 reads them): every
pattern against every record of the given FASTA / FASTQ files (plain or gzip), one TSV row per match:

    pat_id  text_id  cost  strand  start  end  match_region  cigar

Defaults follow the reference: alphabet iupac, reverse complement on, max_n_frac 0.2.  Rows come
text record by text record, patterns in input order (the reference's order depends on its thread
scheduling).

`filter` mirrors `sassy filter` (bin/grep.rs:660-673): the same pattern and searcher arguments; every input record
that holds a match of ANY pattern with cost <= k (`-v / --invert`: that holds none) is written to stdout as it was
read, in input order -- FASTQ records as `@id`, sequence, `+`, quality; FASTA records as `>id` and the sequence on one
line.  It asks `Searcher.best_pattern` for one cost per record: no match records are made.

`search --best` writes at most one row per record: its best match over all patterns and strands (lowest cost, then
the first pattern, then the forward strand, then the rightmost end), through `Searcher.best_matches`.

`search --hamming` counts mismatches only (no insertions or deletions): every start with at most k mismatching positions,
all patterns against all records of a batch in one `Searcher.search_hamming_many` call; rows record by record, inside a
record by (pattern, strand, start).

`demux [-p/-f patterns] -k K [--no-rc] [--max-n-frac F] PATH ...` writes one row per record: the barcode (pattern) with the
fewest mismatches in it, through `Searcher.hamming_best_pattern` (lowest cost, then the first pattern, then the forward
strand, then the leftmost start):

    text_id  pat_id  cost  strand  start

A record that holds no pattern within k mismatches gets `*` for pat_id and strand, and -1 for cost and start.

`count PATTERNS FASTX ... -k K [--rc] [--alphabet A] [--max-n-frac F] [--per-record]` writes how many places every pattern
has at 0, 1, ..., K mismatches per strand -- the table guide and primer design ranks candidates by --, through
`Searcher.hamming_counts_many`: one call per FASTX batch, summed on the host; no match records are made.  PATTERNS is a
FASTA / FASTQ file or a file with one pattern per line (ids 1, 2, ...).  Forward strand only unless `--rc`; no N rule unless
`--max-n-frac`.  A header row, then one row per pattern and scanned strand:

    pat_id  strand  n_0 ... n_K

`--per-record` writes the rows per record instead (one call per record: the per-chromosome table), `text_id` in front.
`--device-unwrap` (with `--per-record`, and on `amplicon`; FASTA only) reads the records through `read_fasta_device_batches`:
the file's bytes go up once, kernels drop headers and line ends, every call gets a device-resident text; the output is the same.
`--device-parse` (on `demux`, and on `count` without `--per-record`; FASTQ only) reads the records through
`read_fastq_device_batches`: a batch's bytes go up once, kernels find and check the reads and lay them out, and the batch call
scans them where they lie (`sassy_amd.DeviceReads`); the output is the same.

`amplicon PRIMERS FASTX ... -k K --min-len A --max-len B [--no-rc] [-a dna|iupac] [--max-n-frac X] [--seq]` writes which
products primer pairs make (in-silico PCR) through `Searcher.hamming_amplicons`, one call per FASTX record.  PRIMERS is a TSV
of `name<TAB>fwd<TAB>rev`, both primers written 5'->3'.  Strand `+`: fwd matches at `start` and the reverse complement of rev
ends at `end`; strand `-` (not with `--no-rc`): the other way round; each primer with at most K mismatches, A <= length <= B,
every combination a row.  A header row, then rows by (record, pair, strand, start, end):

    pair_id  text_id  strand  start  end  length  fwd_cost  rev_cost

`--seq` appends the product's bytes, reverse-complemented for strand `-`.

`pairs A [B] -k K [--rc] [--nearest] [-a dna|iupac|ascii|ascii_ci]` compares sets of equal-length sequences (barcodes, UMIs,
guides) all against all, through `Searcher.hamming_pairs`: which sequence of A is within K mismatches of which sequence of B
(`--rc`: or of its reverse complement, strand `-`); without B, A against itself, every unordered pair once.  A and B load as
`count`'s PATTERNS.  A header row, then rows by (a, b, strand):

    a_id  b_id  strand  cost

`--nearest` writes one row per sequence of A through `Searcher.hamming_nearest` -- its nearest sequence of B (of A: its nearest
other one), and `ties`, how many are that near; `*`, `*` and -1 where nothing is within K:

    a_id  b_id  strand  cost  ties

`--edit` counts K edits (substitutions, insertions and deletions; `Searcher.edit_pairs` / `edit_nearest`) where the rows above
count K mismatches: a barcode that lost or gained a base is then one edit from its origin.  The sequences of B may have a
length of their own; both lengths are at most 64.  Same rows.

`cluster A -k K [--edit] [--rc] [-a dna|iupac|ascii|ascii_ci] [--umi unique|cluster|directional]` writes which groups the sequences of A form, through
`Searcher.hamming_clusters` (`--edit`: `edit_clusters`): the connected components of the graph that joins two sequences within
K of each other (`--rc`: or of each other's reverse complement) -- what `pairs A` lists as records, without the records.  A
loads as `pairs` loads it.  A header row, then one row per sequence in input order; `cluster_id` is the id of the cluster's
first sequence:

    id  cluster_id  cluster_size

`--umi METHOD` groups UMIs through `Searcher.umi_groups` instead (mismatches only): identical sequences are collapsed and
counted, then `unique` stops there, `cluster` takes the components of the distinct sequences and `directional` lets a
sequence absorb a neighbour of at most half its reads (count(a) >= 2 count(b) - 1, UMI-tools' rule).  `rep_id` is the id of
the first sequence identical to the row's, `group_id` the id of the sequence that opened its group, `group_size` in reads:

    id  rep_id  count  group_id  group_size

`overlap R1 R2 [--min-overlap N] [-k K] [--max-permille P] [--alphabet dna|iupac]` writes how the two reads of every pair of
two FASTQ files overlap, through `Searcher.read_overlaps`: read r of R1 against the reverse complement of read r of R2 at
every end-to-end offset; both files are parsed on the device and cut at the same records.  An offset is accepted with at
least N rows of overlap (default 10), at most K mismatches (default: no limit) and at most P per thousand of them (default
200); the best one has the lowest mismatch density.  `accepted` counts the accepted offsets (above 1: repeats); `insert` is
the fragment length and `keep1` / `keep2` what of each read belongs to it (less than the read where the pair reads through
into adapter); all zero offsets and insert 0 where nothing is accepted.  A header row, then one row per pair, the id R1's:

    id  offset  overlap  mismatches  accepted  insert  keep1  keep2

`merge R1 R2 [-o MERGED.fq] [--unmerged1 U1.fq --unmerged2 U2.fq] [--min-overlap N] [-k K] [--max-permille P] [--alphabet
dna|iupac] [--tsv]` merges the two reads of every pair that `overlap` finds an accepted offset for, through
`Searcher.merge_pairs`, on the device: the merged read is R1 up to the overlap, the consensus inside it (equal bases take the
higher quality; of different ones the base of the higher quality wins, R1's on a tie, with quality
min(126, 33 + max(2, |q1 - q2|))) and the reverse complement of R2 behind it; a pair that reads through keeps its overlap
alone.  Merged records go to `-o` (default stdout) under R1's id; pairs without an accepted offset are copied unchanged to
`--unmerged1` / `--unmerged2` where these are given; `--tsv` writes `overlap`'s rows to MERGED.fq.tsv.

`trim IN.fq -a ADAPTER [-a ...] [-o OUT.fq] [-q N] [-m N] [--min-overlap N] [-k K] [--max-permille P] [--alphabet dna|iupac]
[--tsv]` cuts the 3' adapter and the low-quality tail off every read through `Searcher.trim_reads`, on the device: first the
BWA / cutadapt quality rule under `-q` (Phred+33), then the leftmost position at which one of the adapters -- whole, or the
prefix that runs off the read's end -- lies with at least `--min-overlap` rows, at most K mismatches and P per thousand of
them.  Trimmed records go to `-o` (default stdout) under their own ids; reads left shorter than `-m`, or empty, are not
written; `--tsv` writes one row per read to OUT.fq.tsv:

    id  length  quality_len  adapter_pos  adapter  overlap  mismatches

`dedup IN.fq --umi-len N [--at N] [--end3] [-k K] [--method unique|cluster|directional] [--alphabet dna|iupac] -o OUT.fq
[--mate R2.fq --mate-out OUT2.fq] [--tsv FILE]` keeps one read per UMI group through `DeviceReads.dedup`, on the device: the key
of a read is its N bases at distance `--at` from its 5' end (`--end3`: its 3' end), the groups are `cluster --umi`'s over the
keys, and of every group the read with the highest quality sum stays (on a tie the first).  Groups are formed per batch of the
input.  Kept records go to `-o` under their own ids, whole; their mates to `--mate-out`; `--tsv` writes one row per read --
`label_id` the id of the read whose key opened the group (`-`: the read is too short for a key), `size` the group's reads,
`count` the reads that carry the row's key, `kept` 1 for the read that stays:

    read_id  label_id  size  count  kept

`agrep [-i] [-C N] PATTERN K [PATH ...]` mirrors `sassy agrep` (bin/grep.rs:132-307, README "To fuzzy search plain ASCII
files"): every file (no path or `-`: stdin) is read whole and searched forward with the `ascii` profile (`-i`: `ascii_ci`);
one block per match, sorted by (start, end): `PATH:LINE:COL:COST:` and the line(s) the match lies in -- LINE and the line's
bounds come from the device (`Searcher.search_lines`), COL is the 1-based byte column of the match's start.  `-C N` adds up to
N lines of context as `PATH-LINE-` rows, `--` between blocks that do not touch.  The per-cost histogram goes to stderr.
`-E / --classes` reads PATTERN as a class expression (`gr[ae]y`, `\\d\\d\\d\\d-\\d\\d-\\d\\d`, `.`, `[^ ]`; one element per
position, `sassy_amd.parse_classes`) and searches it through `Searcher.search_classes`; with `-i` the sets are closed under case.
Exit status 0: something matched, 1: nothing did, 2: error.

Not mirrored: coloured output, --v2, threads.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Tuple

from . import NO_MATCH, ClassPattern, SassyHipError, Searcher, parse_classes

BATCH_BYTES = 64 << 20  # input bytes per search_many call (a longer record is a batch of its own; the reader reuses its buffers)


# (the reader: sassy_amd/fastx.py -- batches of whole records as one buffer + offsets, numpy over an mmap)
from .fastx import first_byte, read_fasta_device_batches, read_fastq_device_batches, read_fastx, read_fastx_batches  # noqa: E402,F401


def load_patterns(args) -> List[Tuple[str, bytes]]:
    if args.pattern is not None:
        return [("pattern", args.pattern.encode())]          # bin/grep.rs:625-631
    if args.pattern_file is not None:
        with open(args.pattern_file, "rb") as fh:            # one pattern per line, ids 1, 2, ...
            return [(str(i + 1), line.rstrip(b"\r\n")) for i, line in enumerate(fh)]
    if args.pattern_fasta is not None:
        return list(read_fastx(args.pattern_fasta))
    raise SystemExit("No --pattern, --pattern-file, or --pattern-fasta provided!")


def add_search_arguments(sp) -> None:
    """The pattern sources and searcher settings `search` and `filter` share (bin/grep.rs:30-157)."""
    g = sp.add_mutually_exclusive_group()
    g.add_argument("-p", "--pattern")
    g.add_argument("-l", "--pattern-file")
    g.add_argument("-f", "--pattern-fasta")
    sp.add_argument("-k", type=int, required=True)
    sp.add_argument("-a", "--alphabet", type=str.lower, choices=["dna", "iupac", "ascii", "ascii_ci"], default="iupac",
                    help="ascii / ascii_ci (case-insensitive) have no reverse complement: they are searched forward only")
    sp.add_argument("--overhang", type=float, default=None,
                    help="cost per base of overhang alignment in [0, 1] (iupac only); default disabled")
    sp.add_argument("--no-rc", action="store_true")
    sp.add_argument("--max-n-frac", type=float, default=0.2)


def kept_records(cost, invert: bool):
    """Indices of the records `filter` writes: those whose best cost is a match (invert: is NO_MATCH), in input order."""
    import numpy as np
    cost = np.asarray(cost)
    return np.flatnonzero((cost == NO_MATCH) if invert else (cost != NO_MATCH))


def write_records(out, batch, indices) -> None:
    """Records `indices` of a RecordBatch to the binary stream `out` in the reference's shape (bin/grep.rs:660-673)."""
    for i in indices:
        i = int(i)
        quality = batch.quality(i)
        if quality:  # (as the reference: a record with a quality line is written as FASTQ, any other as FASTA)
            out.write(b"@" + batch.id(i).encode() + b"\n" + batch.sequence(i) + b"\n+\n" + quality + b"\n")
        else:
            out.write(b">" + batch.id(i).encode() + b"\n" + batch.sequence(i) + b"\n")


def run_filter(args, searcher, pats, out) -> int:
    for path in args.paths:
        for batch in read_fastx_batches(path, BATCH_BYTES):
            if not len(batch):
                continue
            cost, _, _ = searcher.best_pattern(pats, batch.texts, args.k)
            write_records(out, batch, kept_records(cost, args.invert))
    out.flush()
    return 0


def _line_after(text: bytes, end: int):
    """(start, end) of the line behind the one that ends at `end` (the index of its newline, or len(text)); None at the
    end of the text -- a final newline opens no further line."""
    start = end + 1
    if start >= len(text):
        return None
    stop = text.find(b"\n", start)
    return start, len(text) if stop < 0 else stop


def _line_before(text: bytes, start: int):
    """(start, end) of the line in front of the one that begins at `start`; None at the start of the text."""
    if start == 0:
        return None
    return text.rfind(b"\n", 0, start - 1) + 1, start - 1


def format_agrep(path: str, text: bytes, matches, spans, context: int = 0) -> str:
    """The agrep blocks of one file.  `matches`: records with text_start / text_end / cost; `spans`: their line spans
    (line_no, last_line_no, line_start, line_end; Searcher.search_lines), parallel.  Blocks come by (text_start,
    text_end).  A match row is `PATH:LINE:COL:COST:` and text[line_start:line_end] (a match across a newline shows all its
    lines).  context > 0: up to that many lines in front of and behind the match's lines as `PATH-LINE-` rows, found by
    walking outward from the span; a line is shown as context once and never behind its own match row; `--` stands between
    two blocks whose lines do not touch."""
    order = sorted(range(len(matches)), key=lambda i: (matches[i].text_start, matches[i].text_end))
    out = []
    shown = 0  # the last line number written
    for at, i in enumerate(order):
        m = matches[i]
        line_no, last_line_no = int(spans[i]["line_no"]), int(spans[i]["last_line_no"])
        line_start, line_end = int(spans[i]["line_start"]), int(spans[i]["line_end"])
        before = []
        pos, no = line_start, line_no
        while len(before) < context and no - 1 > shown:
            prev = _line_before(text, pos)
            if prev is None:
                break
            no -= 1
            before.append((no, prev))
            pos = prev[0]
        first_row = before[-1][0] if before else line_no
        if context and shown and first_row > shown + 1:
            out.append("--\n")
        for no, (a, b) in reversed(before):
            out.append(f"{path}-{no}-{text[a:b].decode(errors='replace')}\n")
        col = m.text_start - line_start + 1
        out.append(f"{path}:{line_no}:{col}:{m.cost}:{text[line_start:line_end].decode(errors='replace')}\n")
        shown = max(shown, last_line_no)
        # lines behind the match, up to the next match's own line
        stop_at = int(spans[order[at + 1]]["line_no"]) if at + 1 < len(order) else None
        pos, no = line_end, last_line_no
        for _ in range(context):
            nxt = _line_after(text, pos)
            if nxt is None or (stop_at is not None and no + 1 >= stop_at):
                break
            no += 1
            if no > shown:
                out.append(f"{path}-{no}-{text[nxt[0]:nxt[1]].decode(errors='replace')}\n")
                shown = no
            pos = nxt[1]
    return "".join(out)


def format_histogram(hist) -> str:
    """The per-cost statistics the reference's agrep prints last (bin/grep.rs:309-328), without the bold type."""
    digits = len(str(max(hist, default=0)))
    return (f"\nStatistics: total {sum(hist)}\n"
            "dist: " + "".join(f"{i:>{digits}} " for i in range(len(hist))) + "\n"
            "cnt:  " + "".join(f"{c:>{digits}} " for c in hist) + "\n")


def agrep_parser(sub=None):
    doc = "fuzzy search of plain text files: one block per match, PATH:LINE:COL:COST:line"
    ap = sub.add_parser("agrep", help=doc) if sub is not None else argparse.ArgumentParser(prog="python -m sassy_amd agrep", description=doc)
    ap.add_argument("-i", "--ignore-case", action="store_true", help="the ascii_ci profile: A-Z and a-z match each other")
    ap.add_argument("-C", "--context", type=int, default=0, metavar="N", help="lines of context around every match")
    ap.add_argument("-E", "--classes", action="store_true",
                    help="PATTERN is a class expression, one element per position: gr[ae]y, \\d\\d\\d\\d-\\d\\d, '.', [^ ] "
                         "(sassy_amd.parse_classes; no quantifiers, alternation or anchors)")
    ap.add_argument("pattern")
    ap.add_argument("k", type=int)
    ap.add_argument("paths", nargs="*", help="files to search; none or '-': standard input")
    return ap


def run_agrep(args, stdin=None, out=None, err=None) -> int:
    stdin = sys.stdin.buffer if stdin is None else stdin
    out = sys.stdout if out is None else out
    err = sys.stderr if err is None else err
    if args.k < 0 or args.context < 0:
        err.write("agrep: K and -C must not be negative\n")
        return 2
    pattern = args.pattern.encode()
    hist = [0] * (args.k + 1)
    try:
        if getattr(args, "classes", False):
            pattern = parse_classes(pattern)
        searcher = Searcher("ascii_ci" if args.ignore_case else "ascii", rc=False)
        for path in args.paths or ["-"]:
            if path == "-":
                name, text = "(stdin)", stdin.read()
            else:
                name = path
                with open(path, "rb") as fh:
                    text = fh.read()
            if isinstance(pattern, ClassPattern):
                matches, spans = searcher.search_classes(pattern, text, args.k, lines=True)
            else:
                matches, spans = searcher.search_lines(pattern, text, args.k)
            for m in matches:
                hist[m.cost] += 1
            out.write(format_agrep(name, text, matches, spans, args.context))
    except (OSError, SassyHipError) as e:
        err.write(f"agrep: {e}\n")
        return 2
    out.flush()
    err.write(format_histogram(hist))
    return 0 if sum(hist) else 1


def hamming_rows(searcher, patterns, text_id, where, matches, sam=False):
    """The TSV rows of one record's Hamming hits (Searcher.search_hamming's order: pattern, strand, start); `where` is the
    record's text as format_tsv takes it."""
    return [searcher.format_tsv(m, patterns[m.pattern_idx][0], text_id, where, sam=sam) for m in matches]


def hamming_batch_rows(searcher, patterns, batch, matches, sam=False):
    """The TSV rows of one batch's Hamming hits (Searcher.search_hamming_many's records of batch.texts), in the order the
    per-record calls gave them: record by record, inside a record (pattern, strand, start) -- the call's own order is
    (pattern, strand, record, start), so a stable sort on the record index is all it takes."""
    base = int(batch.texts.buffer.ctypes.data)
    rows = []
    for m in sorted(matches, key=lambda x: x.text_idx):
        ti = m.text_idx
        where = (base + int(batch.texts.starts[ti]), int(batch.texts.lens[ti]))
        rows.extend(hamming_rows(searcher, patterns, batch.id(ti), where, [m], sam=sam))
    return rows


DEMUX_HEADER = "text_id\tpat_id\tcost\tstrand\tstart\n"


def demux_rows(patterns, ids, best):
    """One row per record from Searcher.hamming_best_pattern's four arrays: text_id, pat_id, cost, strand, start; a record
    without a hit: `*` for the pattern and the strand, -1 for cost and start."""
    cost, pattern, strand, start = best
    rows = []
    for i, text_id in enumerate(ids):
        if int(cost[i]) == NO_MATCH:
            rows.append(f"{text_id}\t*\t-1\t*\t-1\n")
        else:
            rows.append(f"{text_id}\t{patterns[int(pattern[i])][0]}\t{int(cost[i])}\t{'-' if int(strand[i]) else '+'}\t{int(start[i])}\n")
    return rows


def run_demux(args, searcher, patterns, out) -> int:
    out.write(DEMUX_HEADER)
    pats = [p for _, p in patterns]
    device_parse = getattr(args, "device_parse", False)  # the reads of a batch are parsed, laid out and scanned on the device
    for path in args.paths:
        for batch in (read_fastq_device_batches if device_parse else read_fastx_batches)(path, BATCH_BYTES):
            if not len(batch):
                continue
            best = searcher.hamming_best_pattern(pats, batch.texts, args.k)
            out.writelines(demux_rows(patterns, [batch.id(i) for i in range(len(batch))], best))
            if device_parse:
                batch.free()
    out.flush()
    return 0


def count_header(k: int, per_record: bool = False) -> str:
    return ("text_id\t" if per_record else "") + "pat_id\tstrand\t" + "\t".join(f"n_{c}" for c in range(k + 1)) + "\n"


def count_rows(patterns, table, rc: bool, text_id=None):
    """The TSV rows of one counts table (Searcher.hamming_counts' shape (n_patterns, 2, k + 1)): per pattern its '+' row and,
    for an rc searcher, its '-' row; text_id in front for --per-record."""
    rows = []
    front = "" if text_id is None else f"{text_id}\t"
    for p, (pat_id, _) in enumerate(patterns):
        for strand in range(2 if rc else 1):
            rows.append(front + f"{pat_id}\t{'-' if strand else '+'}\t" + "\t".join(str(int(v)) for v in table[p][strand]) + "\n")
    return rows


def load_count_patterns(path: str) -> List[Tuple[str, bytes]]:
    """PATTERNS of `count`: FASTA / FASTQ records, or one pattern per line with ids 1, 2, ... (empty lines skipped)."""
    with open(path, "rb") as fh:
        first = fh.read(1)
    if first in (b">", b"@"):
        return list(read_fastx(path))
    with open(path, "rb") as fh:
        lines = [line.rstrip(b"\r\n") for line in fh]
    return [(str(i + 1), line) for i, line in enumerate(line for line in lines if line)]


def run_count(args, searcher, patterns, out) -> int:
    import numpy as np
    pats = [p for _, p in patterns]
    out.write(count_header(args.k, args.per_record))
    total = np.zeros((len(pats), 2, args.k + 1), dtype=np.uint64)
    for path in args.paths:
        if getattr(args, "device_unwrap", False):  # (--per-record only: every record's text stays on the device)
            for batch in read_fasta_device_batches(path, BATCH_BYTES):
                for i in range(len(batch)):
                    out.writelines(count_rows(patterns, searcher.hamming_counts(pats, batch.text(i), args.k), searcher.rc,
                                              text_id=batch.id(i)))
                batch.free()
            continue
        if getattr(args, "device_parse", False):  # (without --per-record: the batch call scans the reads where they lie)
            for batch in read_fastq_device_batches(path, BATCH_BYTES):
                if len(batch):
                    total += searcher.hamming_counts_many(pats, batch.texts, args.k)
                batch.free()
            continue
        for batch in read_fastx_batches(path, BATCH_BYTES):
            if not len(batch):
                continue
            if args.per_record:
                for i in range(len(batch)):
                    out.writelines(count_rows(patterns, searcher.hamming_counts(pats, batch.sequence(i), args.k), searcher.rc,
                                              text_id=batch.id(i)))
            else:
                total += searcher.hamming_counts_many(pats, batch.texts, args.k)
    if not args.per_record:
        out.writelines(count_rows(patterns, total, searcher.rc))
    out.flush()
    return 0


def count_parser(sub):
    cp = sub.add_parser("count", help="write per pattern and strand how many places it has at 0 .. k mismatches as TSV to stdout")
    cp.add_argument("patterns", metavar="PATTERNS", help="FASTA / FASTQ of patterns, or one pattern per line")
    cp.add_argument("paths", metavar="FASTX", nargs="+")
    cp.add_argument("-k", type=int, required=True)
    cp.add_argument("--rc", action="store_true", help="count the reverse complement's places as strand '-' as well")
    cp.add_argument("-a", "--alphabet", type=str.lower, choices=["dna", "iupac", "ascii", "ascii_ci"], default="iupac")
    cp.add_argument("--max-n-frac", type=float, default=None, help="drop places whose span holds a larger fraction of N (default: none dropped)")
    cp.add_argument("--per-record", action="store_true", help="rows per record (text_id in front) instead of summed over all records")
    cp.add_argument("--device-unwrap", action="store_true",
                    help="with --per-record, FASTA only: upload the file's bytes and drop headers and line ends on the device")
    cp.add_argument("--device-parse", action="store_true",
                    help="without --per-record, FASTQ only: upload the file's bytes, find and lay out the reads on the device")
    return cp


def pairs_header(nearest: bool = False) -> str:
    return "a_id\tb_id\tstrand\tcost" + ("\tties" if nearest else "") + "\n"


def pairs_rows(a_seqs, b_seqs, records):
    """The TSV rows of Searcher.hamming_pairs' records: a_id, b_id, strand, cost -- in the records' order."""
    return [f"{a_seqs[int(r['a_idx'])][0]}\t{b_seqs[int(r['b_idx'])][0]}\t{'-' if r['strand'] else '+'}\t{int(r['cost'])}\n" for r in records]


def nearest_rows(a_seqs, b_seqs, cost, index, strand, ties):
    """The TSV rows of Searcher.hamming_nearest's columns, one per sequence of A: b_id and strand are `*` and cost is -1
    where nothing is within k."""
    rows = []
    for i, (a_id, _) in enumerate(a_seqs):
        if int(cost[i]) == NO_MATCH:
            rows.append(f"{a_id}\t*\t*\t-1\t0\n")
        else:
            rows.append(f"{a_id}\t{b_seqs[int(index[i])][0]}\t{'-' if strand[i] else '+'}\t{int(cost[i])}\t{int(ties[i])}\n")
    return rows


def run_pairs(args, searcher, a_seqs, b_seqs, out) -> int:
    a = [s for _, s in a_seqs]
    b = None if b_seqs is None else [s for _, s in b_seqs]
    out.write(pairs_header(args.nearest))
    edit = getattr(args, "edit", False)
    if args.nearest:
        nearest = searcher.edit_nearest if edit else searcher.hamming_nearest
        out.writelines(nearest_rows(a_seqs, a_seqs if b_seqs is None else b_seqs, *nearest(a, b, args.k)))
    else:
        pairs = searcher.edit_pairs if edit else searcher.hamming_pairs
        out.writelines(pairs_rows(a_seqs, a_seqs if b_seqs is None else b_seqs, pairs(a, b, args.k)))
    out.flush()
    return 0


def pairs_parser(sub):
    cp = sub.add_parser("pairs", help="write which sequences of A and B (or of A alone) are within k mismatches of each other as TSV to stdout")
    cp.add_argument("a", metavar="A", help="FASTA / FASTQ of equal-length sequences, or one sequence per line")
    cp.add_argument("b", metavar="B", nargs="?", default=None, help="the second set (left out: A against itself, every unordered pair once)")
    cp.add_argument("-k", type=int, required=True)
    cp.add_argument("--rc", action="store_true", help="compare with the reverse complements of B as strand '-' as well")
    cp.add_argument("--nearest", action="store_true", help="one row per sequence of A: its nearest sequence of B and how many tie with it")
    cp.add_argument("-a", "--alphabet", type=str.lower, choices=["dna", "iupac", "ascii", "ascii_ci"], default="dna")
    cp.add_argument("--edit", action="store_true",
                    help="k edits (substitutions, insertions, deletions) instead of k mismatches; B may have a length of its own, both at most 64")
    return cp


def cluster_header() -> str:
    return "id\tcluster_id\tcluster_size\n"


def cluster_rows(seqs, labels, sizes):
    """The TSV rows of Searcher.hamming_clusters' arrays, one per sequence in input order: its id, the id of its cluster's
    first sequence, the cluster's size."""
    return [f"{seq_id}\t{seqs[int(labels[i])][0]}\t{int(sizes[i])}\n" for i, (seq_id, _) in enumerate(seqs)]


def umi_header() -> str:
    return "id\trep_id\tcount\tgroup_id\tgroup_size\n"


def umi_rows(seqs, labels, sizes, reps, counts):
    """The TSV rows of Searcher.umi_groups' arrays, one per sequence in input order: its id, the id of the first sequence
    identical to it, how many are, the id of the sequence that opened its group, the reads in that group."""
    return [f"{seq_id}\t{seqs[int(reps[i])][0]}\t{int(counts[i])}\t{seqs[int(labels[i])][0]}\t{int(sizes[i])}\n" for i, (seq_id, _) in enumerate(seqs)]


def run_cluster(args, searcher, seqs, out) -> int:
    if args.umi:
        out.write(umi_header())
        out.writelines(umi_rows(seqs, *searcher.umi_groups([s for _, s in seqs], args.k, args.umi)))
        out.flush()
        return 0
    clusters = searcher.edit_clusters if args.edit else searcher.hamming_clusters
    out.write(cluster_header())
    out.writelines(cluster_rows(seqs, *clusters([s for _, s in seqs], args.k)))
    out.flush()
    return 0


def cluster_parser(sub):
    cp = sub.add_parser("cluster", help="write the groups a set of sequences forms (connected components within k) as TSV to stdout")
    cp.add_argument("a", metavar="A", help="FASTA / FASTQ of equal-length sequences, or one sequence per line")
    cp.add_argument("-k", type=int, required=True)
    cp.add_argument("--rc", action="store_true", help="a sequence also joins one whose reverse complement is within k")
    cp.add_argument("-a", "--alphabet", type=str.lower, choices=["dna", "iupac", "ascii", "ascii_ci"], default="dna")
    cp.add_argument("--edit", action="store_true", help="k edits (substitutions, insertions, deletions) instead of k mismatches; sequences of at most 64")
    cp.add_argument("--umi", choices=["unique", "cluster", "directional"], default=None,
                    help="UMI grouping: identical sequences collapsed and counted first; unique: no more than that; cluster: the components of the "
                         "distinct sequences; directional: a sequence absorbs a neighbour of at most (its count + 1) / 2 reads.  Rows: id, rep_id, "
                         "count, group_id, group_size")
    return cp


OVERLAP_HEADER = "id\toffset\toverlap\tmismatches\taccepted\tinsert\tkeep1\tkeep2\n"


def overlap_rows(ids, records, lens1, lens2):
    """The TSV rows of Searcher.read_overlaps' array, one per pair: R1's id, the record, and overlap_trims of it."""
    from . import overlap_trims
    rows = []
    for i, rec in enumerate(records):
        insert, keep1, keep2 = overlap_trims(rec, int(lens1[i]), int(lens2[i]))
        rows.append(f"{ids[i]}\t{int(rec['offset'])}\t{int(rec['overlap'])}\t{int(rec['mismatches'])}\t{int(rec['n_accepted'])}\t{insert}\t{keep1}\t{keep2}\n")
    return rows


def run_overlap(args, searcher, out) -> int:
    from .fastx import read_fastq_pair_device_batches
    out.write(OVERLAP_HEADER)
    for b1, b2 in read_fastq_pair_device_batches(args.r1, args.r2, BATCH_BYTES):
        records = searcher.read_overlaps(b1.texts, b2.texts, args.min_overlap, args.k, args.max_permille)
        out.writelines(overlap_rows([b1.id(i) for i in range(len(b1))], records, b1.texts.seq_lens, b2.texts.seq_lens))
        b1.free()
        b2.free()
    out.flush()
    return 0


def overlap_parser(sub):
    cp = sub.add_parser("overlap", help="write the best overlap of the two reads of every pair (paired-end FASTQ) as TSV to stdout")
    cp.add_argument("r1", metavar="R1", help="FASTQ of the first reads")
    cp.add_argument("r2", metavar="R2", help="FASTQ of the second reads, in the same order")
    cp.add_argument("--min-overlap", type=int, default=10, help="rows an accepted overlap has at least (default 10)")
    cp.add_argument("-k", type=int, default=512, help="mismatches an accepted overlap has at most (default: no limit)")
    cp.add_argument("--max-permille", type=int, default=200, help="mismatches per thousand rows an accepted overlap has at most (default 200)")
    cp.add_argument("-a", "--alphabet", type=str.lower, choices=["dna", "iupac"], default="dna")
    return cp


def run_merge(args, searcher, out) -> int:
    """`merge`: every pair with an accepted overlap as one FASTQ record under R1's id (Searcher.merge_pairs; out: a binary
    stream); the pairs without one go, unchanged, to --unmerged1 / --unmerged2 where these are given."""
    from . import reads_to_fastq
    from .fastx import read_fastq_pair_device_batches
    u1 = open(args.unmerged1, "wb") if args.unmerged1 else None
    u2 = open(args.unmerged2, "wb") if args.unmerged2 else None
    tsv = open(args.tsv_path, "w") if args.tsv_path else None
    try:
        if tsv:
            tsv.write(OVERLAP_HEADER)
        for b1, b2 in read_fastq_pair_device_batches(args.r1, args.r2, BATCH_BYTES, keep_quality=True):
            merged = None
            try:  # (a refused batch -- a read over 512 bases, another letter under dna -- lets go of its device memory as well)
                merged, records = searcher.merge_pairs(b1.texts, b2.texts, args.min_overlap, args.k, args.max_permille, with_overlaps=True)
                ids = [b1.id(i) for i in range(len(b1))]
                out.write(reads_to_fastq(merged, ids))
                if tsv:
                    tsv.writelines(overlap_rows(ids, records, b1.texts.seq_lens, b2.texts.seq_lens))
                for r in (merged.seq_lens == 0).nonzero()[0].tolist():
                    if u1:
                        u1.write(b1.record(r))
                    if u2:
                        u2.write(b2.record(r))
            finally:
                if merged is not None:
                    merged.free()
                b1.free()
                b2.free()
        out.flush()
    finally:
        for fh in (u1, u2, tsv):
            if fh:
                fh.close()
    return 0


def merge_parser(sub):
    cp = sub.add_parser("merge", help="merge the two reads of every pair that overlap (paired-end FASTQ) into one FASTQ record")
    cp.add_argument("r1", metavar="R1", help="FASTQ of the first reads")
    cp.add_argument("r2", metavar="R2", help="FASTQ of the second reads, in the same order")
    cp.add_argument("-o", "--output", default="", help="the merged FASTQ, under R1's ids (default: stdout)")
    cp.add_argument("--unmerged1", default="", help="R1's records of the pairs that were not merged, unchanged")
    cp.add_argument("--unmerged2", default="", help="R2's records of the pairs that were not merged, unchanged")
    cp.add_argument("--min-overlap", type=int, default=10, help="rows an accepted overlap has at least (default 10)")
    cp.add_argument("-k", type=int, default=512, help="mismatches an accepted overlap has at most (default: no limit)")
    cp.add_argument("--max-permille", type=int, default=200, help="mismatches per thousand rows an accepted overlap has at most (default 200)")
    cp.add_argument("-a", "--alphabet", type=str.lower, choices=["dna", "iupac"], default="dna")
    cp.add_argument("--tsv", action="store_true", help="also write `overlap`'s rows, to MERGED.fq.tsv beside -o (needs -o)")
    return cp


TRIM_HEADER = "id\tlength\tquality_len\tadapter_pos\tadapter\toverlap\tmismatches\n"


def trim_rows(ids, records):
    """The TSV rows of Searcher.trim_reads' records, one per read."""
    return [f"{ids[i]}\t{int(r['length'])}\t{int(r['quality_len'])}\t{int(r['adapter_pos'])}\t{int(r['adapter'])}\t{int(r['overlap'])}\t{int(r['mismatches'])}\n"
            for i, r in enumerate(records)]


def run_trim(args, searcher, out) -> int:
    """`trim`: every read cut at its 3' adapter and its low-quality tail, under its own id (Searcher.trim_reads; out: a binary
    stream); a read left shorter than -m is not written."""
    from . import reads_to_fastq
    from .fastx import read_fastq_device_batches
    tsv = open(args.tsv_path, "w") if args.tsv_path else None
    adapters = [a.encode() for a in args.adapter]
    try:
        if tsv:
            tsv.write(TRIM_HEADER)
        for batch in read_fastq_device_batches(args.input, BATCH_BYTES, keep_quality=True):
            trimmed = None
            try:  # (a refused batch lets go of its device memory as well)
                trimmed, records = searcher.trim_reads(batch.texts, adapters, args.min_overlap, args.k, args.max_permille, args.quality_cutoff,
                                                       args.min_length, with_records=True)
                ids = [batch.id(i) for i in range(len(batch))]
                out.write(reads_to_fastq(trimmed, ids))
                if tsv:
                    tsv.writelines(trim_rows(ids, records))
            finally:
                if trimmed is not None:
                    trimmed.free()
                batch.free()
        out.flush()
    finally:
        if tsv:
            tsv.close()
    return 0


def trim_parser(sub):
    cp = sub.add_parser("trim", help="cut the 3' adapter and the low-quality tail off every read of a FASTQ file")
    cp.add_argument("input", metavar="IN.fq", help="FASTQ of the reads")
    cp.add_argument("-a", "--adapter", action="append", default=[], metavar="ADAPTER",
                    help="an adapter, 5'->3' as it follows the insert (up to 64 of 1 .. 64 bases; none: quality and length only)")
    cp.add_argument("-o", "--output", default="", help="the trimmed FASTQ (default: stdout)")
    cp.add_argument("-q", "--quality-cutoff", type=int, default=0, help="Phred quality the 3' end is trimmed below (default 0: not at all)")
    cp.add_argument("-m", "--min-length", type=int, default=0, help="reads left shorter than this are dropped (default 0)")
    cp.add_argument("--min-overlap", type=int, default=3, help="rows of an adapter an accepted position shows at least (default 3)")
    cp.add_argument("-k", type=int, default=512, help="mismatches an accepted position has at most (default: no limit)")
    cp.add_argument("--max-permille", type=int, default=100, help="mismatches per thousand rows an accepted position has at most (default 100)")
    cp.add_argument("--alphabet", type=str.lower, choices=["dna", "iupac"], default="dna")
    cp.add_argument("--tsv", action="store_true", help="also write one row per read from the records, to OUT.fq.tsv beside -o (needs -o)")
    return cp


SPLIT_HEADER = "id\tsample\tbest\tcost\tsecond\tn_best\n"


def split_rows(ids, names, records):
    """The TSV rows of DeviceReads.demux's records, one per read: the sample by its barcode's id, `unassigned` where none."""
    return [f"{ids[i]}\t{names[int(r['sample'])] if int(r['sample']) >= 0 else 'unassigned'}\t{int(r['best']) if int(r['n_best']) else -1}\t"
            f"{int(r['cost'])}\t{int(r['second'])}\t{int(r['n_best'])}\n" for i, r in enumerate(records)]


def split_names(barcodes):
    """The file stems of `split`: the barcodes' ids up to their first blank, which must be distinct, free of path separators and
    none of them `unassigned`."""
    names = [(i.split() or [""])[0] for i, _ in barcodes]
    for n in names:
        if not n or "/" in n or os.sep in n or n in (".", "..") or n == "unassigned" or n.endswith("_2"):
            raise SystemExit(f"split: barcode id {n!r} cannot name a file (empty, a path, `unassigned`, or ending in _2)")
    if len(set(names)) != len(names):
        raise SystemExit("split: the barcode ids must be distinct")
    return names


def run_split(args, searcher, barcodes) -> int:
    """`split`: every read into OUTDIR/<barcode id>.fq without its barcode, or into OUTDIR/unassigned.fq (DeviceReads.demux);
    with --mate the mates, whole, in the same order into <id>_2.fq.  The files are made anew, empty ones included, and every
    batch appends to them."""
    from . import reads_to_fastq
    from .fastx import read_fastq_device_batches, read_fastq_pair_device_batches
    import numpy as np
    names = split_names(barcodes) + ["unassigned"]
    os.makedirs(args.outdir, exist_ok=True)
    suffixes = ("", "_2") if args.mate else ("",)
    for name in names:
        for suf in suffixes:
            open(os.path.join(args.outdir, name + suf + ".fq"), "wb").close()
    tsv = open(os.path.join(args.outdir, "assignments.tsv"), "w") if args.tsv else None
    seqs = [b for _, b in barcodes]

    def append(reads, ids, bounds, suf):
        # one FASTQ of the whole sorted batch, cut at the samples' bounds by the records' sizes
        lens = reads.seq_lens.astype(np.int64)
        sizes = np.where(lens > 0, np.array([len(i.encode()) for i in ids], dtype=np.int64) + 2 * lens + 6, 0)
        ends = np.concatenate([[0], np.cumsum(sizes)])
        data = reads_to_fastq(reads, ids)
        for s, name in enumerate(names):
            a, b = int(ends[int(bounds[s])]), int(ends[int(bounds[s + 1])])
            if b > a:
                with open(os.path.join(args.outdir, name + suf + ".fq"), "ab") as fh:
                    fh.write(data[a:b])

    try:
        if tsv:
            tsv.write(SPLIT_HEADER)
        batches = (read_fastq_pair_device_batches(args.input, args.mate, BATCH_BYTES, keep_quality=True) if args.mate
                   else ((b, None) for b in read_fastq_device_batches(args.input, BATCH_BYTES, keep_quality=True)))
        for b1, b2 in batches:
            d = mates = None
            try:  # (a refused batch lets go of its device memory as well)
                d = b1.texts.demux(searcher, seqs, k=args.k, min_delta=args.min_delta, at=args.at, end3=args.end3, clip=not args.keep_barcode,
                                   with_records=bool(tsv))
                order = d.order.astype(np.int64).tolist()
                ids = [b1.id(i) for i in range(len(b1))]
                append(d.reads, [ids[r] for r in order], d.bounds, "")
                if b2 is not None:
                    mates = b2.texts.select(d.order)
                    ids2 = [b2.id(i) for i in range(len(b2))]
                    append(mates, [ids2[r] for r in order], d.bounds, "_2")
                if tsv:
                    tsv.writelines(split_rows(ids, names, d.records))
            finally:
                for x in (d, mates, b1, b2):
                    if x is not None:
                        x.free()
    finally:
        if tsv:
            tsv.close()
    return 0


def split_parser(sub):
    cp = sub.add_parser("split", help="demultiplex a FASTQ file by sample barcode into one FASTQ file per sample")
    cp.add_argument("input", metavar="IN.fq", help="FASTQ of the reads that carry the barcode")
    cp.add_argument("-f", "--barcodes", required=True, metavar="BARCODES.fa", help="FASTA of the barcodes, all of one length; the ids name the files")
    cp.add_argument("-k", type=int, required=True, help="mismatches an assigned read's barcode has at most")
    cp.add_argument("-o", "--outdir", required=True, metavar="OUTDIR", help="directory of <barcode id>.fq and unassigned.fq")
    cp.add_argument("--mate", default="", metavar="R2.fq", help="FASTQ of the mates, in the same order: written whole to <id>_2.fq")
    cp.add_argument("--at", type=int, default=0, help="bases between the read's end and the barcode (default 0)")
    cp.add_argument("--end3", action="store_true", help="the barcode is counted from the 3' end")
    cp.add_argument("--min-delta", type=int, default=1, help="mismatches the runner-up has at least more than the best (default 1: ties are unassigned)")
    cp.add_argument("--keep-barcode", action="store_true", help="do not clip the barcode off")
    cp.add_argument("--alphabet", type=str.lower, choices=["dna", "iupac"], default="dna")
    cp.add_argument("--tsv", action="store_true", help="also write one row per read from the records, to OUTDIR/assignments.tsv")
    return cp


DEDUP_HEADER = "read_id\tlabel_id\tsize\tcount\tkept\n"


def dedup_rows(ids, label, size, count, kept):
    """The TSV rows of DeviceReads.dedup's columns, one per read: the id of the read that labels its group (`-` where the read
    has no window), the group's reads, the reads that carry its key, and 1 where it is the kept one."""
    is_kept = set(int(r) for r in kept)
    return [f"{ids[r]}\t{ids[int(label[r])] if int(label[r]) != 0xFFFFFFFF else '-'}\t{int(size[r])}\t{int(count[r])}\t{1 if r in is_kept else 0}\n"
            for r in range(len(ids))]


def run_dedup(args, searcher) -> int:
    """`dedup`: of every UMI group of a batch the best read into OUT.fq (DeviceReads.dedup); with --mate the mates of the kept
    reads into --mate-out.  Groups are formed per batch of the input."""
    from . import reads_to_fastq
    from .fastx import read_fastq_device_batches, read_fastq_pair_device_batches
    out = open(args.output, "wb")
    out2 = open(args.mate_out, "wb") if args.mate else None
    tsv = open(args.tsv, "w") if args.tsv else None
    try:
        if tsv:
            tsv.write(DEDUP_HEADER)
        batches = (read_fastq_pair_device_batches(args.input, args.mate, BATCH_BYTES, keep_quality=True) if args.mate
                   else ((b, None) for b in read_fastq_device_batches(args.input, BATCH_BYTES, keep_quality=True)))
        for b1, b2 in batches:
            d = mates = None
            try:  # (a refused batch lets go of its device memory as well)
                d = b1.texts.dedup(searcher, args.umi_len, k=args.k, method=args.method, at=args.at, end3=args.end3, with_columns=bool(tsv))
                kept = d.kept.astype("int64").tolist()
                ids = [b1.id(i) for i in range(len(b1))]
                out.write(reads_to_fastq(d.reads, [ids[r] for r in kept]))
                if b2 is not None:
                    mates = b2.texts.select(d.kept)
                    out2.write(reads_to_fastq(mates, [b2.id(r) for r in kept]))
                if tsv:
                    tsv.writelines(dedup_rows(ids, d.label, d.size, d.count, kept))
            finally:
                for x in (d, mates, b1, b2):
                    if x is not None:
                        x.free()
    finally:
        for fh in (out, out2, tsv):
            if fh:
                fh.close()
    return 0


def dedup_parser(sub):
    cp = sub.add_parser("dedup", help="keep one read per UMI group of a FASTQ file")
    cp.add_argument("input", metavar="IN.fq", help="FASTQ of the reads that carry the UMI")
    cp.add_argument("--umi-len", type=int, required=True, metavar="N", help="bases of the key: the UMI, or the UMI and the first bases behind it (1 .. 128)")
    cp.add_argument("--at", type=int, default=0, help="bases between the read's end and the key (default 0)")
    cp.add_argument("--end3", action="store_true", help="the key is counted from the 3' end")
    cp.add_argument("-k", type=int, default=1, help="mismatches two neighbouring keys have at most (default 1)")
    cp.add_argument("--method", choices=["unique", "cluster", "directional"], default="directional")
    cp.add_argument("--alphabet", type=str.lower, choices=["dna", "iupac"], default="dna")
    cp.add_argument("-o", "--output", required=True, metavar="OUT.fq", help="the kept reads")
    cp.add_argument("--mate", default="", metavar="R2.fq", help="FASTQ of the mates, in the same order")
    cp.add_argument("--mate-out", default="", metavar="OUT2.fq", help="the mates of the kept reads (with --mate)")
    cp.add_argument("--tsv", default="", metavar="FILE", help="also write one row per read: read_id label_id size count kept")
    return cp


def load_primers(path: str) -> List[Tuple[str, bytes, bytes]]:
    """PRIMERS of `amplicon`: rows of name<TAB>fwd<TAB>rev (empty lines and lines from `#` on skipped)."""
    pairs = []
    with open(path, "rb") as fh:
        for no, line in enumerate(fh, 1):
            line = line.rstrip(b"\r\n")
            if not line or line.startswith(b"#"):
                continue
            cols = line.split(b"\t")
            if len(cols) != 3 or not cols[1] or not cols[2]:
                raise SystemExit(f"{path}:{no}: a primer row is name<TAB>fwd<TAB>rev")
            pairs.append((cols[0].decode(), cols[1], cols[2]))
    return pairs


_IUPAC_COMPLEMENT = bytes.maketrans(b"ACTGRYSWKMBDHVNXactgryswkmbdhvnx", b"TGACYRSWMKVHDBNXtgacyrswmkvhdbnx")
_DNA_COMPLEMENT = bytes.maketrans(b"ACTG", b"TGAC")


def product_bytes(alphabet: str, text: bytes, start: int, end: int, strand: int) -> bytes:
    """A product as `--seq` writes it: text[start:end], reverse-complemented for strand 1 under the alphabet's complement."""
    seq = bytes(text[start:end])
    return seq.translate(_DNA_COMPLEMENT if alphabet == "dna" else _IUPAC_COMPLEMENT)[::-1] if strand else seq


AMPLICON_HEADER = "pair_id\ttext_id\tstrand\tstart\tend\tlength\tfwd_cost\trev_cost\n"


def amplicon_rows(pairs, text_id: str, records, alphabet: str = "iupac", text: bytes = None, span=None):
    """The TSV rows of one record's amplicons (Searcher.hamming_amplicons' array, in its order); `text`: append the product;
    `span(start, end)` instead of `text`: the product's bytes from wherever the text lives."""
    rows = []
    for r in records:
        start, end, strand = int(r["start"]), int(r["end"]), int(r["strand"])
        row = f"{pairs[int(r['pair_idx'])][0]}\t{text_id}\t{'-' if strand else '+'}\t{start}\t{end}\t{end - start}\t{int(r['fwd_cost'])}\t{int(r['rev_cost'])}"
        if span is not None:
            row += "\t" + product_bytes(alphabet, span(start, end), 0, end - start, strand).decode("latin-1")
        elif text is not None:
            row += "\t" + product_bytes(alphabet, text, start, end, strand).decode("latin-1")
        rows.append(row + "\n")
    return rows


def run_amplicon(args, searcher, pairs, out) -> int:
    out.write(AMPLICON_HEADER[:-1] + ("\tproduct\n" if args.seq else "\n"))
    primers = [(f, r) for _, f, r in pairs]
    for path in args.paths:
        if getattr(args, "device_unwrap", False):  # the records stay on the device; --seq downloads the product spans only
            for batch in read_fasta_device_batches(path, BATCH_BYTES):
                for i in range(len(batch)):
                    records = searcher.hamming_amplicons(primers, batch.text(i), args.k, args.min_len, args.max_len)
                    span = (lambda a, b, i=i, batch=batch: batch.sequence(i, a, b)) if args.seq else None
                    out.writelines(amplicon_rows(pairs, batch.id(i), records, args.alphabet, span=span))
                batch.free()
            continue
        for batch in read_fastx_batches(path, BATCH_BYTES):
            for i in range(len(batch)):
                text = batch.sequence(i)
                records = searcher.hamming_amplicons(primers, text, args.k, args.min_len, args.max_len)
                out.writelines(amplicon_rows(pairs, batch.id(i), records, args.alphabet, text if args.seq else None))
    out.flush()
    return 0


def amplicon_parser(sub):
    cp = sub.add_parser("amplicon", help="write the products of primer pairs (in-silico PCR) as TSV to stdout")
    cp.add_argument("primers", metavar="PRIMERS", help="TSV of name<TAB>fwd<TAB>rev, both primers 5'->3'")
    cp.add_argument("paths", metavar="FASTX", nargs="+")
    cp.add_argument("-k", type=int, required=True, help="mismatches allowed per primer")
    cp.add_argument("--min-len", type=int, required=True)
    cp.add_argument("--max-len", type=int, required=True)
    cp.add_argument("--no-rc", action="store_true", help="strand '+' only: fwd on the forward strand")
    cp.add_argument("-a", "--alphabet", type=str.lower, choices=["dna", "iupac"], default="iupac")
    cp.add_argument("--max-n-frac", type=float, default=None, help="drop primer sites whose span holds a larger fraction of N (default: none dropped)")
    cp.add_argument("--seq", action="store_true", help="append the product's bytes (reverse-complemented for strand '-')")
    cp.add_argument("--device-unwrap", action="store_true",
                    help="FASTA only: upload the file's bytes and drop headers and line ends on the device (the same output)")
    return cp


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m sassy_amd", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    agrep_parser(sub)
    sp = sub.add_parser("search", help="write all matches as TSV to stdout")
    add_search_arguments(sp)
    sp.add_argument("--sam", action="store_true")
    sp.add_argument("--best", action="store_true",
                    help="at most one row per record: its best match over all patterns and strands (Searcher.best_matches)")
    sp.add_argument("--hamming", action="store_true",
                    help="mismatches only (no insertions or deletions): every start with at most k mismatching positions "
                         "(Searcher.search_hamming_many), all patterns against all records of a batch in one call")
    sp.add_argument("paths", nargs="+")
    fp = sub.add_parser("filter", help="write the records that hold a match (-v: that hold none) to stdout")
    add_search_arguments(fp)
    fp.add_argument("-v", "--invert", action="store_true", help="write the records WITHOUT a match")
    fp.add_argument("paths", nargs="+")
    dp = sub.add_parser("demux", help="write per record the pattern (barcode) with the fewest mismatches as TSV to stdout")
    add_search_arguments(dp)
    dp.add_argument("paths", nargs="+")
    dp.add_argument("--device-parse", action="store_true",
                    help="FASTQ only: upload the file's bytes, find and lay out the reads on the device, scan them where they lie")
    count_parser(sub)
    amplicon_parser(sub)
    pairs_parser(sub)
    cluster_parser(sub)
    overlap_parser(sub)
    merge_parser(sub)
    trim_parser(sub)
    split_parser(sub)
    dedup_parser(sub)
    args = ap.parse_args(argv)
    if args.cmd == "dedup":
        if not 1 <= args.umi_len <= 128 or args.at < 0 or args.k < 0:
            ap.error("dedup takes 1 <= --umi-len <= 128, --at >= 0 and -k >= 0")
        if args.at + args.umi_len > 512:
            ap.error("dedup: --at and --umi-len reach past 512 bases")
        if bool(args.mate) != bool(args.mate_out):
            ap.error("dedup: --mate and --mate-out are given together")
        return run_dedup(args, Searcher(args.alphabet, rc=False))
    if args.cmd == "split":
        if args.k < 0 or args.at < 0 or not 0 <= args.min_delta <= 65:
            ap.error("split takes -k >= 0, --at >= 0 and 0 <= --min-delta <= 65")
        barcodes = list(read_fastx(args.barcodes))
        lens = {len(b) for _, b in barcodes}
        if not 1 <= len(barcodes) <= 4096 or len(lens) != 1 or not 1 <= min(lens) <= 64:
            ap.error("split takes 1 .. 4096 barcodes of one length of 1 .. 64 bases")
        if args.at + min(lens) > 512:
            ap.error("split: --at and the barcode's length reach past 512 bases")
        return run_split(args, Searcher(args.alphabet, rc=False), barcodes)
    if args.cmd == "trim":
        if args.min_overlap < 1 or args.k < 0 or not 0 <= args.max_permille <= 1000 or not 0 <= args.quality_cutoff <= 93 or args.min_length < 0:
            ap.error("trim takes --min-overlap >= 1, -k >= 0, 0 <= --max-permille <= 1000, 0 <= -q <= 93 and -m >= 0")
        if len(args.adapter) > 64 or any(not 1 <= len(a) <= 64 for a in args.adapter):
            ap.error("trim takes up to 64 adapters of 1 .. 64 bases")
        if args.tsv and not args.output:
            ap.error("trim --tsv writes beside the trimmed file: it needs -o")
        args.tsv_path = args.output + ".tsv" if args.tsv else ""
        searcher = Searcher(args.alphabet, rc=False)
        if args.output:
            with open(args.output, "wb") as fh:
                return run_trim(args, searcher, fh)
        return run_trim(args, searcher, sys.stdout.buffer)
    if args.cmd == "merge":
        if args.min_overlap < 1 or args.k < 0 or not 0 <= args.max_permille <= 1000:
            ap.error("merge takes --min-overlap >= 1, -k >= 0 and 0 <= --max-permille <= 1000")
        if args.tsv and not args.output:
            ap.error("merge --tsv writes beside the merged file: it needs -o")
        args.tsv_path = args.output + ".tsv" if args.tsv else ""
        searcher = Searcher(args.alphabet, rc=False)
        if args.output:
            with open(args.output, "wb") as fh:
                return run_merge(args, searcher, fh)
        return run_merge(args, searcher, sys.stdout.buffer)
    if args.cmd == "overlap":
        if args.min_overlap < 1 or args.k < 0 or not 0 <= args.max_permille <= 1000:
            ap.error("overlap takes --min-overlap >= 1, -k >= 0 and 0 <= --max-permille <= 1000")
        return run_overlap(args, Searcher(args.alphabet, rc=False), sys.stdout)
    if getattr(args, "device_parse", False):
        if args.cmd == "count" and args.per_record:
            ap.error("count --device-parse serves the summed table: --per-record takes --device-unwrap (FASTA) or no flag")
        for path in args.paths:
            if first_byte(path) not in (b"@", b""):
                ap.error(f"{args.cmd} --device-parse takes FASTQ only: {path} does not begin with '@'")
    if args.cmd == "cluster":
        if not 0 <= args.k <= 254:
            ap.error("cluster takes 0 <= k <= 254")
        if args.rc and args.alphabet.startswith("ascii"):
            ap.error("cluster --rc: there is no reverse complement of plain text")
        if args.umi and args.edit:
            ap.error("cluster --umi groups by mismatches only: it does not take --edit")
        seqs = load_count_patterns(args.a)
        if not seqs:
            ap.error(f"cluster: {args.a} holds no sequence")
        m = len(seqs[0][1])
        for i, (_, seq) in enumerate(seqs):
            if len(seq) != m:
                ap.error(f"cluster takes sequences of one length: {args.a}: sequence {i} has {len(seq)} bytes, the first has {m}")
        return run_cluster(args, Searcher(args.alphabet, rc=args.rc), seqs, sys.stdout)
    if args.cmd == "pairs":
        if not 0 <= args.k <= 254:
            ap.error("pairs takes 0 <= k <= 254")
        if args.rc and args.alphabet.startswith("ascii"):
            ap.error("pairs --rc: there is no reverse complement of plain text")
        a_seqs = load_count_patterns(args.a)
        b_seqs = None if args.b is None else load_count_patterns(args.b)
        for path, seqs in ((args.a, a_seqs), (args.b, b_seqs)):
            if seqs is not None and not seqs:
                ap.error(f"pairs: {path} holds no sequence")
            # one length for both sets; under --edit one length per set
            first, of = (path, seqs) if args.edit and seqs else (args.a, a_seqs)
            m = len(of[0][1])
            for i, (_, seq) in enumerate(seqs or ()):
                if len(seq) != m:
                    ap.error(f"pairs takes sequences of one length: {path}: sequence {i} has {len(seq)} bytes, the first of {first} has {m}")
        searcher = Searcher(args.alphabet, rc=args.rc)
        return run_pairs(args, searcher, a_seqs, b_seqs, sys.stdout)
    if args.cmd == "amplicon":
        if not 0 <= args.k <= 254:
            ap.error("amplicon takes 0 <= k <= 254")
        if not 1 <= args.min_len <= args.max_len <= (1 << 24):
            ap.error("amplicon takes 1 <= --min-len <= --max-len <= 2^24")
        searcher = Searcher(args.alphabet, rc=not args.no_rc).with_max_n_frac(args.max_n_frac)
        return run_amplicon(args, searcher, load_primers(args.primers), sys.stdout)
    if args.cmd == "count":
        if not 0 <= args.k <= 254:
            ap.error("count takes 0 <= k <= 254")
        if args.rc and args.alphabet.startswith("ascii"):
            ap.error("count --rc: there is no reverse complement of plain text")
        if args.device_unwrap and not args.per_record:
            ap.error("count --device-unwrap needs --per-record: the batch call takes host texts only")
        searcher = Searcher(args.alphabet, rc=args.rc).with_max_n_frac(args.max_n_frac)
        return run_count(args, searcher, load_count_patterns(args.patterns), sys.stdout)
    if args.cmd == "demux" and args.overhang is not None:
        ap.error("demux counts mismatches: it does not take --overhang")
    if args.cmd == "agrep":
        return run_agrep(args)
    if args.cmd == "search" and args.hamming and (args.best or args.overhang is not None):
        ap.error("--hamming takes neither --best nor --overhang")

    patterns = load_patterns(args)
    rc = not args.no_rc and not args.alphabet.startswith("ascii")  # (no reverse complement of plain text: forward only)
    searcher = Searcher(args.alphabet, rc=rc, alpha=args.overhang).with_max_n_frac(args.max_n_frac)
    if args.cmd == "filter":
        return run_filter(args, searcher, [p for _, p in patterns], sys.stdout.buffer)
    if args.cmd == "demux":
        return run_demux(args, searcher, patterns, sys.stdout)
    out = sys.stdout
    out.write("pat_id\ttext_id\tcost\tstrand\tstart\tend\tmatch_region\tcigar\n")
    pats = [p for _, p in patterns]

    import numpy as np

    # every pattern against every record of a batch in one call (the records of a batch are one buffer + offsets:
    # fastx.RecordBatch -- nothing is copied per record, nothing is split but the stream of records into batches);
    # rows record by record, patterns in input order
    for path in args.paths:
        for batch in read_fastx_batches(path, BATCH_BYTES):
            if not len(batch):
                continue
            if args.hamming:  # one call per batch: all patterns, all records
                hits = searcher.search_hamming_many(pats, batch.texts, args.k)
                out.writelines(hamming_batch_rows(searcher, patterns, batch, hits, sam=args.sam))
                continue
            if args.best:  # (one record per text at most, in text order already)
                res = searcher.best_matches(pats, batch.texts, args.k, as_result=True)
            else:
                res = searcher.search_many(pats, batch.texts, args.k, as_result=True)
            arr = res.array
            order = np.lexsort((np.arange(len(arr)), arr["pattern_idx"], arr["text_idx"]))  # stable: keeps each pair's match order
            ms = res.lazy_matches
            base = int(batch.texts.buffer.ctypes.data)
            for i in order.tolist():
                m = ms[i]
                ti = m.text_idx
                where = (base + int(batch.texts.starts[ti]), int(batch.texts.lens[ti]))
                out.write(searcher.format_tsv(m, patterns[m.pattern_idx][0], batch.id(ti), where, sam=args.sam))
    return 0
