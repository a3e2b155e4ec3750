"""A gzip member whose output passes 4 GiB, generated piece by piece and never held whole (test infrastructure):
one fixed block holding a literal 'a' and then groups of eight length-258 / distance-1 matches.  A group is 8 x 13 bits
= 13 bytes; from the second group on every group starts at the same bit offset, so the bulk of the member is one
13-byte pattern repeated.  The footer carries the CRC-32 and ISIZE (mod 2^32) of 'a' * (1 + 2064 * groups)."""
import zlib

from _inflate_edge_cases import fixed_lit, fixed_match

GZ_HEADER = bytes([0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0, 0x03])


class _Bits:
    """LSB-first bit writer that hands out whole bytes as they are done and keeps the rest pending"""

    def __init__(self):
        self.acc, self.n, self.b = 0, 0, bytearray()

    def bits(self, v, k):
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.b.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):  # a Huffman code, MSB first
        for i in range(k - 1, -1, -1):
            self.bits((c >> i) & 1, 1)

    def take(self):
        out, self.b = bytes(self.b), bytearray()
        return out

    def flush(self):
        if self.n:
            self.b.append(self.acc & 255)
            self.acc, self.n = 0, 0
        return self.take()


def output_size(groups):
    return 1 + 2064 * groups


def _group(w):
    for _ in range(8):
        fixed_match(w, 258, 1)


def raw_chunks(groups, reps=1 << 14):
    """the raw deflate stream (one final fixed block), in pieces of at most 13 * reps bytes"""
    assert groups >= 2
    w = _Bits()
    w.bits(1, 1)  # BFINAL
    w.bits(1, 2)  # BTYPE = fixed
    fixed_lit(w, ord("a"))
    _group(w)
    yield w.take()
    _group(w)
    pat = w.take()  # the pending bits are again what they were before this group
    assert len(pat) == 13
    left = groups - 2
    yield pat
    while left:
        k = min(left, reps)
        yield pat * k
        left -= k
    fixed_lit(w, 256)
    yield w.flush()


def crc_of_output(groups):
    n, crc, block = output_size(groups), 0, b"a" * (1 << 20)
    while n:
        k = min(n, len(block))
        crc = zlib.crc32(block[:k], crc)
        n -= k
    return crc


def gzip_chunks(groups, reps=1 << 14):
    yield GZ_HEADER
    yield from raw_chunks(groups, reps)
    yield crc_of_output(groups).to_bytes(4, "little") + (output_size(groups) & 0xFFFFFFFF).to_bytes(4, "little")


class ChunkReader:
    """a reader over a chunk generator; `on_read` is called before every read"""

    def __init__(self, chunks, on_read=None):
        self._it, self._buf, self.pos, self.on_read = iter(chunks), b"", 0, on_read

    def read(self, n=-1):
        if self.on_read:
            self.on_read(self)
        while len(self._buf) < n:
            nxt = next(self._it, None)
            if nxt is None:
                break
            self._buf += nxt
        out, self._buf = self._buf[:n], self._buf[n:]
        self.pos += len(out)
        return out
