"""Shared by the GPU tests of the text-search side: mixed-case English-like prose with punctuation, digits, bytes >= 0x80,
'_@[' and newlines; the fold the ascii_ci expectations are built on; a text placed on the device."""

WORDS = [b"the", b"Quick", b"BROWN", b"fox", b"Jumps", b"over", b"LAZY", b"dog", b"Error", b"WARNING", b"timeout", b"Kernel",
         b"memory", b"Device", b"ReSeT", b"queue", b"x", b"Zz", b"I", b"at"]
PUNCT = [b" ", b" ", b" ", b", ", b". ", b"\n", b"_", b"@", b"[", b"]", b"`", b"{", b"~", b"^", b"-", b"0", b"17", b"2026",
         b"\xc3\xa9", b"\xe9", b"\xc9", b"\x80", b"\xff", b"\xdf"]


def fold(x: bytes) -> bytes:
    return bytes(x).lower()


def prose(rng, n):
    out = bytearray()
    while len(out) < n:
        w = rng.choice(WORDS)
        r = rng.random()
        out += w.upper() if r < 0.2 else w.lower() if r < 0.4 else w
        out += rng.choice(PUNCT)
    return bytes(out[:n])


class DevText:
    """Minimal stand-in for a CUDA tensor: data_ptr / numel / is_cuda."""

    def __init__(self, ptr, n):
        self._p, self._n, self.is_cuda = ptr, n, True

        class _DT:
            itemsize = 1
        self.dtype = _DT()

    def data_ptr(self):
        return self._p

    def numel(self):
        return self._n

    def is_contiguous(self):
        return True


def on_device(sassy, text):
    buf = sassy.DeviceBuffer(len(text) + 256)
    buf.upload(text)
    return buf, DevText(buf.ptr, len(text))
