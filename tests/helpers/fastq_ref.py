"""The definition of the FASTQ parse on the device (sassy_hip_fastq_parse, sassy_amd.DeviceReads): strict four-line FASTQ.

  * split at '\\n'; a final empty piece is no line;
  * strip one trailing '\\r' from each line;
  * with L lines, record r is lines 4r .. 4r + 3: line 4r begins with '@' and the id is the rest of it, line 4r + 1 is the
    sequence, line 4r + 2 begins with '+' and its content is ignored, line 4r + 3 is the quality (its length is reported,
    not compared).

Nothing else is touched: case, N, an '@' or '+' that opens a quality line, a '\\r' elsewhere.  Empty input is valid.  A record
is malformed if its line 4r lacks the '@' or its line 4r + 2 lacks the '+'; if L is no multiple of 4 the last record, L // 4,
is malformed.  Malformed raises with the smallest malformed record and the rule it breaks; inside one record a missing '@'
comes first, then the missing lines, then a missing '+'.

`parse` is the definition, line by line.  `columns` is the same table with numpy for inputs of millions of records
(tests/test_fastq_reads_cpu.py holds the two against each other); `layout` / `layout_np` are the device text, `rem` the
per-block table of the batch scan.
"""
import random
from typing import List, NamedTuple

import numpy as np

NO_AT, SHORT, NO_PLUS = "does not begin with '@'", "of its four lines", "does not begin with '+'"


class Malformed(ValueError):
    def __init__(self, record: int, rule: str):
        super().__init__(f"record {record}: {rule}")
        self.record, self.rule = record, rule


class Read(NamedTuple):
    id_start: int    # in the raw bytes: the id without '@' and without the line's trailing '\r'
    id_len: int
    seq_start: int   # in the laid-out text: the rounded-up lengths in front of it
    seq: bytes
    qual_start: int  # in the raw bytes
    qual_len: int

    @property
    def seq_len(self) -> int:
        return len(self.seq)


def lines_of(raw: bytes):
    """[(start, line without its line end)]"""
    lines, at = [], 0
    for piece in bytes(raw).split(b"\n"):
        lines.append((at, piece))
        at += len(piece) + 1
    if lines and lines[-1][1] == b"":
        lines.pop()
    return [(at, line[:-1] if line.endswith(b"\r") else line) for at, line in lines]


def parse(raw: bytes) -> List[Read]:
    lines = lines_of(raw)
    out, start = [], 0
    for r in range((len(lines) + 3) // 4):
        rec = lines[4 * r:4 * r + 4]
        if not rec[0][1].startswith(b"@"):
            raise Malformed(r, NO_AT)
        if len(rec) < 4:
            raise Malformed(r, SHORT)
        if not rec[2][1].startswith(b"+"):
            raise Malformed(r, NO_PLUS)
        seq = rec[1][1]
        out.append(Read(rec[0][0] + 1, len(rec[0][1]) - 1, start, seq, rec[3][0], len(rec[3][1])))
        start += (len(seq) + 63) // 64 * 64
    return out


def layout(reads: List[Read]) -> bytes:
    """The device text: every sequence from its seq_start on, zero pads, 64 zero bytes behind the last."""
    total = (reads[-1].seq_start + (len(reads[-1].seq) + 63) // 64 * 64) if reads else 0
    out = bytearray(total + 64)
    for r in reads:
        out[r.seq_start:r.seq_start + len(r.seq)] = r.seq
    return bytes(out)


def records(raw: bytes):
    """[(id, sequence, quality)] as read_fastx_batches gives them."""
    raw = bytes(raw)
    return [(raw[r.id_start:r.id_start + r.id_len].decode(), r.seq, raw[r.qual_start:r.qual_start + r.qual_len]) for r in parse(raw)]


def table(reads: List[Read]):
    """The columns of sassy_hip_ReadRecord as uint64 arrays."""
    col = lambda f: np.array([f(r) for r in reads], dtype=np.uint64)  # noqa: E731
    return {"id_start": col(lambda r: r.id_start), "id_len": col(lambda r: r.id_len), "seq_start": col(lambda r: r.seq_start),
            "seq_len": col(lambda r: r.seq_len), "qual_start": col(lambda r: r.qual_start), "qual_len": col(lambda r: r.qual_len)}


def columns(raw):
    """`table(parse(raw))` and the position of every sequence in raw, with numpy: (columns, seq_src).  Raises Malformed alike."""
    a = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw
    n = a.size
    nl = np.flatnonzero(a == 10).astype(np.int64)
    starts = np.concatenate([np.zeros(1, dtype=np.int64), nl + 1])
    ends = np.concatenate([nl, np.array([n], dtype=np.int64)])
    if starts[-1] >= n:
        starts, ends = starts[:-1], ends[:-1]
    lens = ends - starts
    has_cr = (lens > 0) & (a[np.maximum(ends - 1, 0)] == 13)
    lens = lens - has_cr
    L = starts.size
    first = np.where(lens > 0, a[np.minimum(starts, max(n - 1, 0))], 0) if L else np.zeros(0, dtype=np.uint8)
    bad = np.full(L, False)
    bad[0::4] = first[0::4] != ord("@")
    bad[2::4] = first[2::4] != ord("+")
    bad_line = int(np.flatnonzero(bad)[0]) if bad.any() else None
    cut = L // 4 if L % 4 else None
    if bad_line is not None and (cut is None or bad_line // 4 < cut or (bad_line // 4 == cut and bad_line % 4 == 0)):
        raise Malformed(bad_line // 4, NO_AT if bad_line % 4 == 0 else NO_PLUS)
    if cut is not None:
        raise Malformed(cut, SHORT)
    u = lambda x: x.astype(np.uint64)  # noqa: E731
    seq_len = u(lens[1::4])
    slot = (seq_len + np.uint64(63)) // np.uint64(64) * np.uint64(64)
    cols = {"id_start": u(starts[0::4] + 1), "id_len": u(lens[0::4] - 1), "seq_start": np.cumsum(slot) - slot, "seq_len": seq_len,
            "qual_start": u(starts[3::4]), "qual_len": u(lens[3::4])}
    return cols, starts[1::4]


def layout_np(raw, cols, seq_src) -> np.ndarray:
    """The device text of `columns(raw)` as a uint8 array."""
    a = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw
    seq_len, seq_start = cols["seq_len"].astype(np.int64), cols["seq_start"].astype(np.int64)
    total = int(seq_start[-1] + (seq_len[-1] + 63) // 64 * 64) if seq_len.size else 0
    out = np.zeros(total + 64, dtype=np.uint8)
    if seq_len.size and seq_len.sum():
        rec = np.repeat(np.arange(seq_len.size), seq_len)
        inside = np.arange(int(seq_len.sum()), dtype=np.int64) - np.repeat(np.cumsum(seq_len) - seq_len, seq_len)
        out[seq_start[rec] + inside] = a[np.asarray(seq_src, dtype=np.int64)[rec] + inside]
    return out


def rem(seq_starts, seq_lens) -> np.ndarray:
    """Per 64-byte block of the layout the bytes from its first byte to the end of its own read (hamming_step.h: ham_rem of
    the read ham_text_of names), block by block."""
    seq_starts, seq_lens = [int(x) for x in seq_starts], [int(x) for x in seq_lens]
    total = (seq_starts[-1] + (seq_lens[-1] + 63) // 64 * 64) if seq_starts else 0
    out = np.zeros(total // 64, dtype=np.uint32)
    for s, n in zip(seq_starts, seq_lens):
        for b in range(s // 64, (s + n + 63) // 64):
            out[b] = min(s + n - 64 * b, 0xFFFFFFFF)
    return out


# ---------------------------------------------------------------- the inputs the CPU and the GPU tests share
def corpus():
    """{name: bytes} of valid strict four-line FASTQ."""
    rng = random.Random(11)
    seq = lambda n: bytes(rng.choice(b"ACGTNacgt") for _ in range(n))  # noqa: E731
    qual = lambda n: bytes(rng.choice(b"!#+5@IJ") for _ in range(n))  # noqa: E731
    rec = lambda i, s, eol=b"\n", plus=b"+": b"@" + i + eol + s + eol + plus + eol + qual(len(s)) + eol  # noqa: E731
    files = {
        "empty.fq": b"",
        "one.fq": b"@r1 first\nACGTN\n+\nIIII#\n",
        "one_no_final_newline.fq": b"@r1 first\nACGTN\n+\nIIII#",
        "crlf.fq": b"".join(rec(b"c%d x" % i, seq(n), b"\r\n") for i, n in enumerate([5, 70, 1, 64, 63])),
        "mixed_eol.fq": b"@a\r\nACGT\n+\r\nIIII\r\n@b x\nGG\r\n+b x\nII\n@c\r\nT\r\n+\r\nI",
        "cr_last.fq": b"@a\nACGT\n+\nIII\r",
        "cr_inside.fq": b"@a\rb\nAC\rGT\r\r\n+\r\r\nI\rII\rI\n",
        "quality_opens_with_at_and_plus.fq": b"@a\nACGT\n+\n@III\n@b\nACGT\n+\n+III\n@c\nAC\n+\n@+\n@d\nA\n+\n@\n",
        "plus_repeats_id.fq": b"@read/1 lane=3\nACGTACGT\n+read/1 lane=3\nIIIIIIII\n@r2\nAC\n+r2\nII\n",
        "empty_ids.fq": b"@\nAC\n+\nII\n@\r\nGT\n+\nII\n@\nT\n+\nI\n",
        "empty_sequences.fq": b"@e0\n\n+\n\n@e1\n\n+\n\n@r\nACG\n+\nIII\n@e2\r\n\r\n+\r\n\r\n@e3\n\n+\n\n@s\nT\n+\nI\n@e4\n\n+\n\n@e5\n\n+\n\n",
        "only_empty_sequences.fq": b"@e0\n\n+\n\n@e1\n\n+\n\n",
        "reads.fq": b"".join(rec(b"read%d" % i, seq(rng.randrange(1, 200))) for i in range(500)),
    }
    return files


def malformed():
    """{name: (bytes, smallest malformed record, rule)}"""
    ok = [b"@r%d\nACGT%s\n+\nIIII%s\n" % (i, b"A" * i, b"I" * i) for i in range(6)]
    whole = b"".join(ok)
    lines = whole.split(b"\n")[:-1]
    cut = lambda k: b"\n".join(lines[:k]) + b"\n"  # noqa: E731
    return {
        "lines_4r_plus_1.fq": (cut(4 * 3 + 1), 3, SHORT),
        "lines_4r_plus_2.fq": (cut(4 * 3 + 2), 3, SHORT),
        "lines_4r_plus_3.fq": (cut(4 * 5 + 3), 5, SHORT),
        "lines_2.fq": (b"@a\nAC", 0, SHORT),
        "blank_line_inside.fq": (b"".join(ok[:2]) + b"\n" + b"".join(ok[2:]), 2, NO_AT),
        "blank_line_at_the_end.fq": (whole + b"\n", 6, NO_AT),
        "no_at_record_0.fq": (b"r0" + whole[1:], 0, NO_AT),
        "no_at_middle.fq": (b"".join(ok[:3]) + b"r3" + ok[3][1:] + b"".join(ok[4:]), 3, NO_AT),
        "no_at_last.fq": (b"".join(ok[:5]) + b">" + ok[5][1:], 5, NO_AT),
        "no_plus.fq": (b"".join(ok[:4]) + ok[4].replace(b"\n+\n", b"\n-\n") + ok[5], 4, NO_PLUS),
        "no_plus_in_a_cut_record.fq": (b"".join(ok[:2]) + b"@x\nAC\nII\n", 2, SHORT),
        "wrapped_sequence.fq": (ok[0] + b"@w\nACGT\nACGT\n+\nIIIIIIII\n" + ok[1], 1, NO_PLUS),
    }
