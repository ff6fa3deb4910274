"""The definition of the FASTA unwrap (sassy_hip_fasta_unwrap, sassy_amd.DeviceFasta): the line-by-line parse.

  * split at '\\n'; a final empty piece is no line;
  * strip one trailing '\\r' from each line;
  * a line that begins with '>' opens a record, its id is the rest of that line;
  * every other line is appended to the open record's sequence.

Nothing else is touched: case, N, a '>' that does not begin a line, a '\\r' that is not in front of '\\n' or at the input's end.
The input is empty or begins with '>'.
"""
from typing import List, NamedTuple


class Record(NamedTuple):
    id_start: int   # in the raw bytes: the id without '>' and without the line's trailing '\r'
    id_len: int
    seq_start: int  # in the laid-out text: the rounded-up lengths in front of it
    seq: bytes

    @property
    def seq_len(self) -> int:
        return len(self.seq)


def parse(raw: bytes) -> List[Record]:
    raw = bytes(raw)
    assert not raw or raw[:1] == b">", "the input is empty or begins with '>'"
    lines, at = [], 0
    for piece in raw.split(b"\n"):
        lines.append((at, piece))
        at += len(piece) + 1
    if lines and lines[-1][1] == b"":
        lines.pop()
    found = []
    for at, line in lines:
        if line.endswith(b"\r"):
            line = line[:-1]
        if line.startswith(b">"):
            found.append([at + 1, len(line) - 1, []])
        else:
            found[-1][2].append(line)
    out, start = [], 0
    for id_start, id_len, parts in found:
        seq = b"".join(parts)
        out.append(Record(id_start, id_len, start, seq))
        start += (len(seq) + 63) // 64 * 64
    return out


def layout(records: List[Record]) -> bytes:
    """The device text: every sequence from its seq_start on, zero pads, 64 zero bytes behind the last."""
    total = (records[-1].seq_start + (len(records[-1].seq) + 63) // 64 * 64) if records else 0
    out = bytearray(total + 64)
    for r in records:
        out[r.seq_start:r.seq_start + len(r.seq)] = r.seq
    return bytes(out)


def ids_and_sequences(raw: bytes):
    """[(id, sequence)] as read_fastx gives them."""
    raw = bytes(raw)
    return [(raw[r.id_start:r.id_start + r.id_len].decode(), r.seq) for r in parse(raw)]
