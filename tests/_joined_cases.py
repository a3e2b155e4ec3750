"""Cases of joined compress (flate_hip_compress_joined) and what they must compress to.  A stream of N bytes is cut into
P = max(1, ceil(N / piece)) pieces; every piece is compressed with no history; the stream is the container's header,
F(piece_0) .. F(piece_{P-2}), L(piece_{P-1}) and the container's footer over the WHOLE input, where L(x) is the raw stream
the reference writes for x and F(x) is what a fresh raw reference compressor has written after write(x); flush()
(include/flate_hip.h).  expected() says so with tests/_oracle.py; tests/test_joined_cases_cpu.py holds the expectations
against stdlib zlib, tests/test_gpu_joined.py runs every case on the GPU."""
import numpy as np

import _oracle as O
from flate_amd import synth

LEVELS = (4, 6, 9)
CONTAINERS = (O.RAW, O.GZIP, O.ZLIB)
PIECES = (7, 4096, 65535)
MAX_PIECE = 65535
KINDS = ("text", "noise", "sym64")

TEXT = synth.text(synth.SEED_TEXT, 6 * 65535).tobytes()
NOISE = np.random.default_rng(11).integers(0, 256, 6 * 65535, dtype=np.uint8).tobytes()   # its blocks go out stored
SYM64 = np.random.default_rng(12).integers(0, 64, 6 * 65535, dtype=np.uint8).tobytes()    # a token a byte: 65535 bytes are two blocks

_SOURCE = {"text": TEXT, "noise": NOISE, "sym64": SYM64}


def content(kind, n, at=0):
    return _SOURCE[kind][at: at + n]


def pieces_of(data, piece):
    return [data[a: a + piece] for a in range(0, len(data), piece)] or [b""]


_F, _L = {}, {}


def flushed(x, level):
    """F(x): a fresh raw reference compressor after write(x); flush()"""
    key = (x, level)
    if key not in _F:
        d = O.Deflate(O.RAW, level)
        d.write(x)
        d.flush()
        _F[key] = d.output()
        d.close()
    return _F[key]


def finished(x, level):
    """L(x): the raw stream of x"""
    key = (x, level)
    if key not in _L:
        _L[key] = O.compress(x, O.RAW, level)
    return _L[key]


def marker_bytes(x, level):
    """4 or 5: how much longer F(x) is than L(x)"""
    return len(flushed(x, level)) - len(finished(x, level))


def expected(data, piece, container, level):
    """the bytes flate_hip_compress_joined must write for `data` in pieces of `piece` bytes"""
    ps = pieces_of(data, piece)
    body = b"".join(flushed(p, level) for p in ps[:-1]) + finished(ps[-1], level)
    if container == O.RAW:
        return body
    if container == O.GZIP:
        return (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + O.crc32(data).to_bytes(4, "little") +
                (len(data) & 0xffffffff).to_bytes(4, "little"))
    assert container == O.ZLIB
    return b"\x78\x9c" + body + O.adler32(data).to_bytes(4, "big")


def lengths(piece):
    """the stream lengths of the parity batch; pieces of 65535 bytes stop at 2 * piece + 1"""
    ls = [0, 1, piece - 1, piece, piece + 1, 2 * piece, 2 * piece + 1, 5 * piece + 3]
    return ls[:-1] if piece == MAX_PIECE else ls


def batch(piece):
    """[(name, data)]: every length of lengths(piece) with text, noise and the 64-symbol bytes -- at piece 65535 the latter's
    streams of 2 * piece (+ 1) bytes hold two-block pieces, not last and last"""
    out = []
    for i, n in enumerate(lengths(piece)):
        for j, kind in enumerate(KINDS):
            out.append(("%s_%d" % (kind, n), content(kind, n, at=131 * i + 17 * j)))
    return out


def block_count(x, level):
    """token blocks the reference writes for x"""
    d = O.Deflate(O.RAW, level, log_tokens=True)
    d.write(x)
    d.finish()
    n = len(d.blocks())
    d.close()
    return n


def q1_inputs(level):
    """Inputs whose 32768th token is a match next to a stored block (quirk Q1), built as
    tests/test_gpu_compress.py::_q1_inputs builds its `lost` and `twice` ones: every one a piece's worth (< 65535 bytes)."""
    def covered(data, ntok):
        pos = 0
        for t in O.tokenize(data, level)[:ntok]:
            t = int(t)
            pos += ((t >> 15) & 0xFF) + 3 if (t >> 23) & 1 else 1
        return pos

    out = {}
    for seed in (0, 1):
        a = np.random.default_rng(seed).integers(0, 256, 33000, dtype=np.uint8).tobytes()
        out["lost%d" % seed] = a[:covered(a, 32767)] + a[100:140] + (b"compressible tail " * 2000)[:30000]
        h = np.random.default_rng(seed).integers(0, 64, 40000, dtype=np.uint8).tobytes()
        out["twice%d" % seed] = (h[:covered(h, 32767)] + h[200:216] +
                                 np.random.default_rng(1000 + seed).integers(0, 256, 600, dtype=np.uint8).tobytes())
    return out


def q1_streams(level):
    """[(name, data, piece)]: every Q1 input as a piece that is not the stream's last (text follows) and as the last one
    (text of a piece's length goes first)"""
    out = []
    for name, x in q1_inputs(level).items():
        assert len(x) <= MAX_PIECE
        out.append((name + "_first", x + TEXT[:3000], len(x)))
        out.append((name + "_last", TEXT[5000: 5000 + len(x)] + x, len(x)))
    return out
