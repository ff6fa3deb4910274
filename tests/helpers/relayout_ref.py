"""The two batch layouts search_many scans, in numpy: what layout_texts (sassy_amd/csrc/scan_driver.hip) writes for a host list
of sequences, and so what the relayout kernel (reads_relayout.hip, relayout_step.h) must write for the same reads resident on
the device.  Also the resident batch's own layout (every read from a multiple of 64 on, zeros between, 64 spare bytes)."""
import numpy as np

# the length list: blocks of 16 and 64 from either side, empty reads first in a run, inside and last, one long read
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 0, 4097, 0]
# In that list, in either order and from read 3 on, the lengths in front of any read sum to 0, 1 or 2 mod 16 (the gaps are
# multiples of 16), so no start of the separator layout falls on residue 15 mod 16 or 63 mod 64.  This list adds them: with a
# gap of 32 its starts are 0, 47, 127, 223, 256, 288, 353, 515, 547.
MORE_LENGTHS = [15, 48, 64, 1, 0, 33, 130, 0, 7]


def sequences(lengths, seed=11):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()) for n in lengths]


def separator_starts(lens, gap):
    """search_many_batched: `gap` pad bytes between two texts, none in front of the first or behind the last"""
    starts, at = [], 0
    for i, n in enumerate(lens):
        if i:
            at += gap
        starts.append(at)
        at += n
    return np.array(starts, dtype=np.uint64), at


def pertext_starts(lens, steps):
    """search_many_pertext: every text in whole blocks of its own, `steps` virtual columns behind it"""
    starts, at = [], 0
    for n in lens:
        starts.append(at)
        at += (n + steps + 63) // 64 * 64
    return np.array(starts, dtype=np.uint64), at


def geometries(lens):
    """(name, starts, total, pad) of the four geometries the tests lay `lens` out in"""
    out = []
    for gap in (32, 48):
        s, t = separator_starts(lens, gap)
        out.append(("separator gap %d" % gap, s, t, ord("X")))
    for steps, pad in ((0, "X"), (26, "N")):
        s, t = pertext_starts(lens, steps)
        out.append(("per text steps %d" % steps, s, t, ord(pad)))
    return out


def layout(seqs, starts, total, pad):
    dst = np.full(total, pad, dtype=np.uint8)
    for s, at in zip(seqs, starts.tolist()):
        dst[at:at + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return dst


def resident(seqs):
    """(buffer, seq_starts) of the resident batch: fastq_ref.layout's rule"""
    starts, at = [], 0
    for s in seqs:
        starts.append(at)
        at += (len(s) + 63) // 64 * 64
    buf = np.zeros(at + 64, dtype=np.uint8)
    for s, a in zip(seqs, starts):
        buf[a:a + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return buf, np.array(starts, dtype=np.uint64)


def first_difference(got, want, starts, first=0):
    """None, or a message that names the first differing byte and the read it lies in (or behind)"""
    diff = np.flatnonzero(got != want)
    if not diff.size:
        return None
    at = int(diff[0])
    i = int(np.searchsorted(starts, at, side="right")) - 1
    return "first differing byte %d of %d (block %d, residue %d mod 16): got %d, want %d, in or behind read %d (destination start %d)" % (
        at, want.size, at // 64, at % 16, int(got[at]), int(want[at]), first + max(i, 0), int(starts[max(i, 0)]))
