"""The inputs of the checksum tests (test_checksum_cpu, test_gpu_checksums): contents x lengths, generated, nothing stored
(test infrastructure).  The lengths sit where the CRC-32 / Adler-32 code of the library changes its mind: the 16-byte loads
and their alignment heads, a lane's share of a block (1024), Adler-32's deferred modulo (5552 bytes) and its modulus (65521),
the block unit (65535) and the span path's item (65536), a lane's share of a wave-per-stream (64 x 5552) and a
workgroup-per-stream (1024 x 5552) checksum crossing one Adler round, a lane's run of blocks in the fold becoming two blocks
(64 / 65 x 65535), and a stream of 4097 blocks and a byte.  The reference of every test is Python's zlib on these bytes."""
import zlib

import numpy as np

FP_THREADS = 1024  # threads of k_inflate_par (kernels_inflate_par.h)
BLOCK = 65535

_CENTRES = (0, 1, 16, 1024, 5552, 65521, 65535, 65536, 64 * 1024, 64 * 5552, FP_THREADS * 5552, 64 * BLOCK, 65 * BLOCK,
            4097 * BLOCK + 1)
LENGTHS = sorted({c + d for c in _CENTRES for d in (-1, 0, 1) if c + d >= 0})
CONTENTS = ("ff", "zero", "random", "one_first", "one_last", "ff_zero_mid")
OFFSETS = tuple(range(16))  # byte offset of the plain bytes in the buffer a kernel sees


def make(content, n, seed=0):
    """n bytes of the named content"""
    if content == "ff":
        return b"\xff" * n
    if content == "zero":
        return bytes(n)
    if content == "random":
        return np.random.default_rng(1000003 * seed + n).bytes(n)
    b = bytearray(b"\xff" * n if content == "ff_zero_mid" else n)
    if n:
        if content == "one_first":
            b[0] = 1
        elif content == "one_last":
            b[-1] = 1
        elif content == "ff_zero_mid":
            b[n // 2] = 0
        else:
            raise ValueError(content)
    return bytes(b)


def lengths(lo=0, hi=None):
    return [n for n in LENGTHS if n >= lo and (hi is None or n <= hi)]


def cases(lo=0, hi=None, contents=CONTENTS):
    """(name, content, length) of every case with lo <= length <= hi"""
    return [("%s-%d" % (c, n), c, n) for n in lengths(lo, hi) for c in contents]


def crc32(data):
    return zlib.crc32(data) & 0xFFFFFFFF


def adler32(data):
    return zlib.adler32(data) & 0xFFFFFFFF


def reference(container, data):
    """zlib's CRC-32 (container 1, gzip) or Adler-32 (container 2, zlib) of the plain bytes"""
    return crc32(data) if container == 1 else adler32(data)


def gzip_footer(data):
    return crc32(data).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little")


def zlib_footer(data):
    return adler32(data).to_bytes(4, "big")


def footer(container, data):
    return gzip_footer(data) if container == 1 else zlib_footer(data)


FOOTER_BYTES = {1: 8, 2: 4}
GZ_HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3])
ZL_HEADER = bytes([0x78, 0x9C])


def stored_stream(data):
    """raw deflate of `data` in stored blocks of at most 65535 bytes (five header bytes each; RFC 1951 3.2.4)"""
    out = bytearray()
    n = len(data)
    pos = 0
    while True:
        k = min(BLOCK, n - pos)
        last = pos + k == n
        out += bytes([1 if last else 0]) + k.to_bytes(2, "little") + (k ^ 0xFFFF).to_bytes(2, "little")
        out += data[pos:pos + k]
        pos += k
        if last:
            return bytes(out)


def wrap(container, raw, data, flip_bit=None):
    """header + raw deflate + footer from zlib of `data`; flip_bit: that bit of the footer's checksum is wrong"""
    f = bytearray(footer(container, data))
    if flip_bit is not None:
        f[(flip_bit // 8) % 4] ^= 1 << (flip_bit % 8)
    return (GZ_HEADER if container == 1 else ZL_HEADER) + raw + bytes(f)


# ---- CRC-32 / Adler-32 of a concatenation, from the definitions (for lengths nobody can allocate)
POLY = 0xEDB88320  # reflected: bit 31 is x^0


def gf2_mulmod(a, b):
    """a(x) * b(x) mod P(x), reflected representation"""
    p = 0
    for _ in range(32):
        if a & 0x80000000:
            p ^= b
        a = (a << 1) & 0xFFFFFFFF
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


def gf2_xpow(e):
    """x^e mod P by square and multiply"""
    r, sq = 0x80000000, 0x40000000  # x^0, x^1
    while e:
        if e & 1:
            r = gf2_mulmod(r, sq)
        sq = gf2_mulmod(sq, sq)
        e >>= 1
    return r


def combine(container, a, b, len_b):
    """the checksum of A || B from checksum(A), checksum(B) and |B|"""
    if container == 1:
        return gf2_mulmod(a, gf2_xpow(8 * len_b)) ^ b
    a1, b1, a2, b2 = a & 0xFFFF, a >> 16, b & 0xFFFF, b >> 16
    return ((a1 + a2 - 1) % 65521) | (((b1 + b2 + len_b * (a1 - 1)) % 65521) << 16)
