"""Host-side mirror of the reference's public interface (src/flate.zig:9-71,
src/gzip.zig:4-66, src/zlib.zig:4-66): the same names, argument meaning and error
behaviour, over the C ABI of libflate_hip.so.

  compress(reader, writer, options)     flate.zig:28-30   (one-shot: compressor + compress + finish)
  Compressor / compressor(writer, opt)  flate.zig:33-40   (write / compress / finish; flush: see below)
  decompress(reader, writer)            flate.zig:10-12
  Decompressor / decompressor(reader)   flate.zig:15-22   (decompress / next / read / reader / reset / set_reader)
  decompress_members(data)              -- (not in the reference: all concatenated members in one GPU call)
  build_index(data, spacing=None)       -- (not in the reference: a seek index; StreamIndex.read_at(offset, n))
  huffman.{compress,Compressor,compressor}   flate.zig:44-56
  store.{compress,Compressor,compressor}     flate.zig:59-71
  Options(level=Level.default), Level   deflate.zig:15-32

`reader` is anything with .read() (or a bytes-like), `writer` anything with .write().
Errors are FlateError subclasses named after the reference's error set
(inflate.zig:72-78, huffman_decoder.zig:35-40, container.zig:45-51, bit_reader.zig:29).

Scope of this round: one-shot streams of any length.  At levels 4..9 an
input longer than 65535 bytes is compressed as ONE stream by the whole-stream path
(SURVEY.md 8f-2), byte-identical to the reference's sliding-window compressor.
Compressor.flush (deflate.zig:335-337; 474-478 for the huffman-only / store-only
compressors) is a sync flush that keeps the LZ history.  It is incremental: the object
keeps only the tail of what was written that the reference's window, slide schedule and
pending block can still depend on (from a 32 KiB-aligned position at least 96 KiB before
the previous flush), compresses that tail with its flush points on the GPU and hands the
writer the bytes that follow what the previous flush produced; the container checksum is
folded piece by piece.
"""
import enum
import io

from . import _capi
from .engine import default_engine


class Level(enum.IntEnum):  # deflate.zig:23-32
    fast = 4
    level_4 = 4
    level_5 = 5
    default = 6
    level_6 = 6
    level_7 = 7
    level_8 = 8
    best = 9
    level_9 = 9


class Options:  # deflate.zig:15-17
    def __init__(self, level=Level.default, repair_q1=False):
        self.level = Level(level)
        self.repair_q1 = bool(repair_q1)  # not in the reference: FLATE_HIP_DEFLATE_REPAIR_Q1 (ReferenceQ1StreamWarning)


class FlateError(Exception):
    status = None


def _mk(name, code):
    return type(name, (FlateError,), {"status": code})


EndOfStream = _mk("EndOfStream", 1)
BadGzipHeader = _mk("BadGzipHeader", 2)
BadZlibHeader = _mk("BadZlibHeader", 3)
WrongGzipChecksum = _mk("WrongGzipChecksum", 4)
WrongGzipSize = _mk("WrongGzipSize", 5)
WrongZlibChecksum = _mk("WrongZlibChecksum", 6)
InvalidCode = _mk("InvalidCode", 7)
OversubscribedHuffmanTree = _mk("OversubscribedHuffmanTree", 8)
IncompleteHuffmanTree = _mk("IncompleteHuffmanTree", 9)
MissingEndOfBlockCode = _mk("MissingEndOfBlockCode", 10)
InvalidMatch = _mk("InvalidMatch", 11)
InvalidBlockType = _mk("InvalidBlockType", 12)
WrongStoredBlockNlen = _mk("WrongStoredBlockNlen", 13)
InvalidDynamicBlockHeader = _mk("InvalidDynamicBlockHeader", 14)
OutputTooSmall = _mk("OutputTooSmall", 100)
ChunkTooLarge = _mk("ChunkTooLarge", 101)
InvalidState = _mk("InvalidState", 103)  # inflate.zig:303 (a host-side state, no device status)
NeedDict = _mk("NeedDict", 106)    # a zlib stream with FDICT set, decoded without zdict= (not in the reference)
WrongDict = _mk("WrongDict", 107)  # ... its DICTID is not the Adler-32 of zdict


class ReferenceQ1StreamWarning(UserWarning):
    """The stream just written is byte for byte the reference's -- and does not inflate to its input: the reference flushes
    a full block of 32768 tokens before its window has advanced over the last token's match (deflate.zig:227-230 before
    :193), and when exactly one of the two blocks at that seam is stored the match's bytes are lost or written twice
    (include/flate_hip.h: FLATE_HIP_ST_REFERENCE_Q1_STREAM).  `Options(level, repair_q1=True)` writes a stream that
    inflates to the input instead."""

_ERRORS = {e.status: e for e in (
    EndOfStream, BadGzipHeader, BadZlibHeader, WrongGzipChecksum, WrongGzipSize, WrongZlibChecksum, InvalidCode,
    OversubscribedHuffmanTree, IncompleteHuffmanTree, MissingEndOfBlockCode, InvalidMatch, InvalidBlockType,
    WrongStoredBlockNlen, InvalidDynamicBlockHeader, OutputTooSmall, ChunkTooLarge, NeedDict, WrongDict)}


def raise_for_status(code):
    if code:
        raise _ERRORS.get(code, FlateError)(_capi.status_name(code))


def _compress_status(code):
    """Status of a compress call: 102 is the reference's own (broken) stream -- written as the reference writes it, with a
    warning; anything else non-zero raises."""
    if code == _capi.ST_REFERENCE_Q1_STREAM:
        import warnings
        warnings.warn(ReferenceQ1StreamWarning(ReferenceQ1StreamWarning.__doc__.split("\n")[0]), stacklevel=3)
        return
    raise_for_status(code)


def _read_all(reader):
    if isinstance(reader, (bytes, bytearray, memoryview)):
        return bytes(reader)
    return reader.read()


_HEADERS = {_capi.RAW: b"", _capi.GZIP: bytes([0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0, 0x03]), _capi.ZLIB: bytes([0x78, 0x9C])}
_KEEP = 98304   # history a piece after a flush can depend on: 64 KiB window + one 32 KiB slide step
_STEP = 32768


class _Compressor:
    """Deflate (deflate.zig:121-373) / SimpleCompressor (:449-529) seen from the caller.

    One-shot use (write / compress, then finish) is one GPU call over the whole input.  With flush()
    (deflate.zig:335-337: pending tokens out, then an empty stored block; the LZ history stays) the
    object works INCREMENTALLY: what the reference emits for the bytes after a flush point F depends
    only on the stream from a 32 KiB-aligned position B <= F - 96 KiB on (its 64 KiB window has slid
    past everything older, and the slide schedule is periodic in 32 KiB), so each flush() / finish()
    runs flate_hip_compress_flush on the retained tail [B, now) only and hands the writer the bytes
    after the previous flush's marker.  Cost per flush: O(new bytes + 128 KiB), memory: the tail.
    The container header is written once, the footer's checksum is folded from per-piece checksums
    (flate_hip_checksum / _combine)."""

    def __init__(self, container, mode, writer, engine=None, repair_q1=False):
        self._container, self._mode, self._wrt = container, int(mode), writer
        self._eng = engine or default_engine()
        self._repair = bool(repair_q1)
        self._buf = bytearray()  # stream bytes from absolute position self._base on
        self._base = 0
        self._total = 0          # bytes written so far
        self._flushes = []       # absolute flush points >= self._base
        self._nflush = 0         # flush() calls so far
        self._rel_emitted = None  # bytes the tail [base, last flush) compresses to (cached while base stands)
        self._cks, self._cks_pos = None, 0
        self._done = False

    def _call(self, fn, *args):
        # (the flag is the handle's: set for this object's calls only)
        if not self._repair:
            return fn(*args)
        self._eng.set_flags(_capi.DEFLATE_REPAIR_Q1)
        try:
            return fn(*args)
        finally:
            self._eng.set_flags(0)

    def _live(self):
        # the reference's compressor has no such check (writing after finish() emits a broken stream);
        # the mirror refuses instead of handing the writer bytes that do not extend the finished stream
        if self._done:
            raise InvalidState("compressor used after finish()")

    def write(self, data):  # deflate.zig:363-367
        self._live()
        self._buf += data
        self._total += len(data)
        return len(data)

    def compress(self, reader):  # deflate.zig:304-321
        self._live()
        data = _read_all(reader)
        self._buf += data
        self._total += len(data)

    def writer(self):  # deflate.zig:369-371
        return self

    def _fold_checksum(self):
        """checksum of everything written so far (gzip / zlib footer), piece by piece"""
        if self._container == _capi.RAW:
            return
        new = bytes(self._buf[self._cks_pos - self._base:])
        v = self._eng.checksum(new, self._container)
        self._cks = v if self._cks is None else self._eng.checksum_combine(self._container, self._cks, v, len(new))
        self._cks_pos = self._total

    def _run_tail(self, finish):
        """compress the retained tail with its flush points (raw container); returns the new bytes"""
        rel = [f - self._base for f in self._flushes]
        tail = bytes(self._buf)
        if self._rel_emitted is None:
            # how much of the tail's output was handed over already: the tail up to the previous flush
            prev = rel[-2] if not finish else rel[-1]
            done, st = self._call(self._eng.compress_flush, tail[:prev], rel[:-1] if not finish else rel, False, _capi.RAW, self._mode)
            _compress_status(st)
            self._rel_emitted = len(done)
        out, st = self._call(self._eng.compress_flush, tail, rel, finish, _capi.RAW, self._mode)
        _compress_status(st)
        new = out[self._rel_emitted:]
        self._rel_emitted = len(out)
        return new

    def _drop_history(self):
        last = self._flushes[-1]
        nb = ((last - _KEEP) // _STEP) * _STEP
        if nb > self._base:
            del self._buf[: nb - self._base]
            self._flushes = [f for f in self._flushes if f >= nb]
            self._base = nb
            self._rel_emitted = None

    def flush(self):  # deflate.zig:335-337: pending tokens out, then an empty stored block; history stays
        self._live()
        self._fold_checksum()
        first = self._nflush == 0
        self._flushes.append(self._total)
        self._nflush += 1
        if first:
            self._rel_emitted = 0
            self._wrt.write(_HEADERS[self._container])
        self._wrt.write(self._run_tail(False))
        self._drop_history()

    def set_writer(self, new_writer):  # deflate.zig:351-354
        self._wrt = new_writer

    def finish(self):  # deflate.zig:344-347
        if self._done:
            return
        if self._nflush:
            self._fold_checksum()
            self._wrt.write(self._run_tail(True))
            if self._container == _capi.GZIP:  # container.zig:92-96
                self._wrt.write(self._cks.to_bytes(4, "little") + (self._total & 0xFFFFFFFF).to_bytes(4, "little"))
            elif self._container == _capi.ZLIB:  # container.zig:104
                self._wrt.write(self._cks.to_bytes(4, "big"))
        else:
            outs, st = self._call(self._eng.compress_many, [bytes(self._buf)], self._container, self._mode)
            _compress_status(st[0])
            self._wrt.write(outs[0])
        self._done = True


class _PieceCompressor:
    """SimpleCompressor (deflate.zig:449-529) in bounded memory: writes are gathered into pieces of `piece` bytes, each
    goes to a resumable compressor on the device (flate_hip_deflater_*) and the blocks it completes go to the writer at
    once.  The bytes are those of _Compressor for the same write / flush / finish calls.  Host memory: the piece and
    one output slot, whatever the stream's length."""

    def __init__(self, container, mode, writer, engine=None, piece=1 << 20):
        if int(piece) < 1:
            raise ValueError("piece must be at least 1 byte")
        self._eng = engine or default_engine()
        self._wrt, self._piece = writer, int(piece)
        self._slot = self._piece + 5 * (self._piece // 65535) + (1 << 17)
        self._d = self._eng.deflater(1, container, int(mode))
        self._buf = bytearray()
        self._done = False

    def _feed(self, data, op):
        # the stream never has output pending when a step starts (it is drained below): the piece is taken at once
        outs, st, cons = self._d.feed([data], op=op, caps=self._slot)
        if cons[0] != len(data):
            raise InvalidState("the resumable compressor did not take its piece")
        self._wrt.write(outs[0])
        while st[0] == _capi.ST_NEED_OUTPUT:
            outs, st, _ = self._d.feed([b""], op=_capi.FEED_MORE, caps=self._slot)
            self._wrt.write(outs[0])
        _compress_status(st[0] if op == _capi.FEED_FINISH else 0)

    def _live(self):
        if self._done:
            raise InvalidState("compressor used after finish()")

    def write(self, data):  # deflate.zig:495-511
        self._live()
        mv = memoryview(data).cast("B")
        n = len(mv)
        while len(mv):
            take = min(self._piece - len(self._buf), len(mv))
            self._buf += mv[:take]
            mv = mv[take:]
            if len(self._buf) == self._piece:
                self._feed(bytes(self._buf), _capi.FEED_MORE)
                self._buf.clear()
        return n

    def compress(self, reader):  # deflate.zig:304-321, the reader `piece` bytes at a time
        self._live()
        if isinstance(reader, (bytes, bytearray, memoryview)):
            self.write(reader)
            return
        while True:
            b = reader.read(self._piece - len(self._buf))
            if not b:
                return
            self.write(b)

    def writer(self):
        return self

    def flush(self):  # deflate.zig:474-478
        self._live()
        self._feed(bytes(self._buf), _capi.FEED_FLUSH)
        self._buf.clear()

    def set_writer(self, new_writer):
        self._wrt = new_writer

    def finish(self):  # deflate.zig:480-484
        if self._done:
            return
        self._feed(bytes(self._buf), _capi.FEED_FINISH)
        self._buf.clear()
        self._done = True
        self._d.close()


def _zdict_for(container, zdict):
    """zdict= of the decompress functions: None, or the preset dictionary as bytes (raw and zlib only)"""
    if zdict is None:
        return None
    if container == _capi.GZIP:
        raise ValueError("gzip has no preset dictionaries: zdict= is for flate and zlib")
    return bytes(zdict)


class _Decompressor:
    """Inflate (inflate.zig:43-355) seen from the caller.  The reader is consumed as far as the current stream
    needs it, in steps that double: a decode that runs out of input (EndOfStream) while the reader still has
    bytes is repeated with twice as much -- the input read past the end of a stream stays buffered for reset()
    (inflate.zig:301-309), and the GPU work is at most twice that of the final decode."""

    CHUNK = 65536  # the reference hands out at most its 64 KiB ring per next() (inflate.zig:322-336)
    FIRST_READ = 1 << 16

    def __init__(self, container, reader, engine=None, flags=0, zdict=None):
        self._container, self._flags = container, flags
        self._eng = engine or default_engine()
        self._zdict = _zdict_for(container, zdict)  # a preset dictionary, for every stream of the reader
        self._set_input(reader)
        self._out = None   # decoded bytes of the current stream
        self._rp = 0
        self._ended = False

    def _set_input(self, reader):
        if isinstance(reader, (bytes, bytearray, memoryview)):
            reader = io.BytesIO(bytes(reader))
        self._rd = reader
        self._in = bytearray()  # bytes read from the reader and not yet given up
        self._pos = 0           # start of the current stream in _in
        self._eof = False

    def _fill(self, want):
        """Have `want` bytes of the current stream buffered, or the reader at its end."""
        while not self._eof and len(self._in) - self._pos < want:
            got = self._rd.read(want - (len(self._in) - self._pos))
            if not got:
                self._eof = True
                break
            self._in += got

    def _decode(self):
        if self._out is not None:
            return
        if self._pos > (1 << 20):  # drop what earlier streams consumed
            del self._in[:self._pos]
            self._pos = 0
        want = self.FIRST_READ
        while True:
            self._fill(want)
            data = bytes(self._in[self._pos:])
            cap = max(1 << 16, len(data) * 64)
            while True:
                if self._zdict is None:
                    outs, st, used = self._eng.decompress_many([data], self._container, self._flags, caps=[cap])
                else:
                    outs, st, used = self._eng.decompress_many_dict([data], [self._zdict], None, self._container,
                                                                    self._flags, caps=[cap])
                if st[0] == 100 and cap < (1 << 34):
                    cap *= 8
                    continue
                break
            if st[0] == 1 and not self._eof:  # EndOfStream with input still to come: not an error yet
                want = 2 * max(want, len(data))
                continue
            break
        raise_for_status(st[0])
        self._out, self._used = outs[0], used[0]

    def get(self, limit=0):  # inflate.zig:326-336
        self._decode()
        n = len(self._out) - self._rp
        n = min(n, limit if limit else self.CHUNK)
        buf = self._out[self._rp:self._rp + n]
        self._rp += n
        if n == 0:
            self._ended = True
        return buf

    def next(self):  # inflate.zig:315-319
        buf = self.get(0)
        return buf if buf else None

    def read(self, n=-1):  # inflate.zig:343-347 (n < 0: read to the end, Python convention)
        if n is None or n < 0:
            self._decode()
            buf = self._out[self._rp:]
            self._rp = len(self._out)
            self._ended = True
            return buf
        return self.get(n) if n else b""

    def reader(self):  # inflate.zig:349-351
        return self

    def decompress(self, writer):  # inflate.zig:292-296
        while True:
            buf = self.next()
            if buf is None:
                break
            writer.write(buf)

    def reset(self):  # inflate.zig:301-309: next stream of the same reader
        if not self._ended:
            raise InvalidState("reset() before the end of the stream")
        self._pos += self._used
        self._out, self._rp, self._ended = None, 0, False

    def more_input(self):
        """True when input is left after the stream just decoded (a further concatenated member)."""
        self._decode()
        if self._pos + self._used >= len(self._in):
            self._fill(self._used + 1)
        return self._pos + self._used < len(self._in)

    def set_reader(self, new_reader):  # inflate.zig:283-288
        self._set_input(new_reader)
        self._out, self._rp, self._ended = None, 0, False


class _PieceDecompressor:
    """Inflate (inflate.zig:43-355) in bounded memory: a one-stream inflater on the device (flate_hip_inflater_*) is fed
    the reader `piece` bytes at a time and output is handed out as it is decoded, at most 64 KiB a next()
    (inflate.zig:322-336).  A piece is read only when everything read before has been absorbed, so the reader is never
    more than one piece ahead of the decoder; what the current member does not absorb belongs to the next one (reset()).
    Memory: the piece, one 64 KiB output slot and the device-side state, whatever the stream's length."""

    CHUNK = 65536

    def __init__(self, container, reader, engine=None, flags=0, piece=1 << 20, zdict=None):
        if int(piece) < 1:
            raise ValueError("piece must be at least 1 byte")
        self._container, self._piece = container, int(piece)
        self._eng = engine or default_engine()
        self._zdict = _zdict_for(container, zdict)
        self._slot = min(max(self.CHUNK, 4 * self._piece), 64 << 20)  # output of one feed (handed out 64 KiB at a time)
        self._inf = self._eng.inflater(1, container, flags)
        self._set_input(reader)
        self._clear()
        self._give_dict()

    def _give_dict(self):
        """the preset dictionary again: the device drops it with every reset"""
        if self._zdict is not None and not self._inf.set_dictionary([0], self._zdict)[0]:
            raise InvalidState("the resumable inflater did not take its dictionary")

    def _set_input(self, reader):
        if isinstance(reader, (bytes, bytearray, memoryview)):
            reader = io.BytesIO(bytes(reader))
        self._rd = reader
        self._in = b""    # read from the reader and not absorbed yet
        self._eof = False

    def _clear(self):
        self._out = bytearray()  # decoded, not handed out yet
        self._done = False       # the member is complete (footer checked)
        self._ended = False      # ... and everything of it has been handed out

    def _step(self):
        """one feed: more output, or the end of the member"""
        if not self._in and not self._eof:
            self._in = bytes(self._rd.read(self._piece) or b"")
            self._eof = not self._in
        outs, st, used = self._inf.feed([self._in], final=[self._eof], caps=[self._slot])
        self._in = self._in[used[0]:]
        self._out += outs[0]
        if st[0] == 0:
            self._done = True
        elif st[0] not in (_capi.ST_NEED_INPUT, _capi.ST_NEED_OUTPUT):
            raise_for_status(st[0])

    def get(self, limit=0):  # inflate.zig:326-336
        want = min(limit, self.CHUNK) if limit else self.CHUNK
        while not self._out and not self._done:
            self._step()
        buf = bytes(self._out[:want])
        del self._out[:len(buf)]
        if not buf:
            self._ended = True
        return buf

    def next(self):  # inflate.zig:315-319
        buf = self.get(0)
        return buf if buf else None

    def read(self, n=-1):  # inflate.zig:343-347 (n < 0: read to the end, Python convention)
        if n is None or n < 0:
            parts = []
            while True:
                buf = self.next()
                if buf is None:
                    return b"".join(parts)
                parts.append(buf)
        return self.get(n) if n else b""

    def reader(self):  # inflate.zig:349-351
        return self

    def decompress(self, writer):  # inflate.zig:292-296
        while True:
            buf = self.next()
            if buf is None:
                break
            writer.write(buf)

    def reset(self):  # inflate.zig:301-309: next stream of the same reader
        if not self._ended:
            raise InvalidState("reset() before the end of the stream")
        self._inf.reset([0])
        self._clear()
        self._give_dict()

    def more_input(self):
        """True when input is left after the stream just decoded (a further concatenated member).  Meant for the end of
        a member, after next() has returned None: called earlier, it decodes the rest of the current member first and
        keeps that output buffered for next() -- host memory of the member's remaining output, not O(piece + slot)."""
        while not self._done:
            self._step()
        if not self._in and not self._eof:
            self._in = bytes(self._rd.read(self._piece) or b"")
            self._eof = not self._in
        return bool(self._in)

    def set_reader(self, new_reader):  # inflate.zig:283-288
        self._set_input(new_reader)
        self._inf.reset([0])
        self._clear()
        self._give_dict()


class _Simple:
    """huffman / store namespaces (flate.zig:44-71)."""

    def __init__(self, container, mode):
        self._container, self._mode = container, mode

    def compress(self, reader, writer, engine=None, *, piece=None, joined=None):
        if joined is not None and joined is not False:
            raise ValueError("joined= is for levels 4..9: the huffman and store namespaces have no joined streams")
        c = self.compressor(writer, engine, piece=piece)
        c.compress(reader)
        c.finish()

    def compressor(self, writer, engine=None, *, piece=None):
        """piece=None: the whole-stream compressor.  piece=N: bounded memory -- the input goes to a resumable
        compressor N bytes at a time and its blocks reach the writer as they are made (_PieceCompressor)."""
        if piece is None:
            return _Compressor(self._container, self._mode, writer, engine)
        return _PieceCompressor(self._container, self._mode, writer, engine, piece=piece)

    Compressor = compressor


class ContainerModule:
    """One of flate (raw) / gzip / zlib: identical function set (readme.md:104-124)."""

    def __init__(self, container):
        self._container = container
        self.huffman = _Simple(container, _capi.MODE_HUFFMAN)
        self.store = _Simple(container, _capi.MODE_STORE)
        self.Options, self.Level = Options, Level

    def compress(self, reader, writer, options=None, engine=None, *, piece=None, zdict=None, joined=None, index=None):
        """zdict=: a preset dictionary (flate and zlib only, gzip raises ValueError): the stream is what
        zlib.decompressobj(wbits, zdict=zdict) and decompress(..., zdict=zdict) inflate (flate_hip_compress_batch_dict).
        Its last min(len, 32768) bytes and the input may be 65535 bytes together, else ValueError.
        joined=True, or a piece size of 1..65535: ONE stream of independent pieces (65535 bytes for True) at the rate of
        the chunk path, whatever the input's length (flate_hip_compress_joined); exclusive with piece= and zdict=.
        index=True, or a spacing in bytes (with joined= only): the call returns the blob (bytes) of a seek index over the
        stream it wrote -- its points are piece starts and carry no windows (flate_hip_compress_joined_indexed); True is
        the default spacing, 1 MiB.  index_from_bytes(blob, stream) reads ranges from it.  Otherwise None is returned."""
        zdict = _zdict_for(self._container, zdict)  # (gzip: ValueError, before an engine is made)
        want_index = index is not None and index is not False
        if want_index and (joined is None or joined is False):
            raise ValueError("index= needs joined=: only a stream of independent pieces has window-free points")
        if joined is not None and joined is not False:
            if piece is not None or zdict is not None:
                raise ValueError("joined= takes neither piece= nor zdict=")
            size = _capi.JOIN_MAX_PIECE if joined is True else int(joined)
            if not 1 <= size <= _capi.JOIN_MAX_PIECE:
                raise ValueError("joined= is True or a piece size of 1..%d" % _capi.JOIN_MAX_PIECE)
            options = options or Options()
            data = _read_all(reader)
            eng = engine or default_engine()
            if options.repair_q1:  # (the flag is the handle's: set for this call only, as _Compressor does)
                eng.set_flags(_capi.DEFLATE_REPAIR_Q1)
            try:
                if want_index:
                    spacing = 0 if index is True else int(index)
                    if spacing < 0:
                        raise ValueError("index= is True or a spacing of at least 1 byte")
                    outs, st, ix = eng.compress_joined([data], self._container, int(options.level), piece=size, index_spacing=spacing)
                else:
                    outs, st = eng.compress_joined([data], self._container, int(options.level), piece=size)
            finally:
                if options.repair_q1:
                    eng.set_flags(0)
            blob = None
            if want_index:
                try:
                    blob = eng.index_export(ix)
                finally:
                    eng.index_destroy(ix)
            _compress_status(st[0])
            writer.write(outs[0])
            return blob
        if zdict is not None:
            if piece is not None:
                raise ValueError("piece= takes no zdict=")
            options = options or Options()
            data = _read_all(reader)
            if min(len(zdict), 32768) + len(data) > _capi.DICT_MAX_STREAM:
                raise ValueError("with zdict= the dictionary's last 32768 bytes and the input may be %d bytes together: "
                                 "got %d + %d" % (_capi.DICT_MAX_STREAM, min(len(zdict), 32768), len(data)))
            eng = engine or default_engine()
            if options.repair_q1:  # (the flag is the handle's: set for this call only, as _Compressor does)
                eng.set_flags(_capi.DEFLATE_REPAIR_Q1)
            try:
                outs, st = eng.compress_many_dict([data], [zdict], None, self._container, int(options.level))
            finally:
                if options.repair_q1:
                    eng.set_flags(0)
            _compress_status(st[0])
            writer.write(outs[0])
            return
        c = self.compressor(writer, options, engine, piece=piece)
        c.compress(reader)
        c.finish()

    def compressor(self, writer, options=None, engine=None, *, piece=None):
        """piece=N: bounded memory (_PieceCompressor); only huffman-only and store-only streams are resumable, a
        level 4..9 compressor with piece= raises ValueError."""
        options = options or Options()
        if piece is not None:
            raise ValueError("piece= needs the huffman or store namespace: levels 4..9 are not resumable")
        return _Compressor(self._container, int(options.level), writer, engine, repair_q1=options.repair_q1)

    Compressor = compressor

    def decompress(self, reader, writer, engine=None, *, zdict=None):
        self.decompressor(reader, engine, zdict=zdict).decompress(writer)

    def decompressor(self, reader, engine=None, *, piece=None, zdict=None):
        """piece=None: the whole-stream decompressor.  piece=N: bounded memory -- the reader is read N bytes at a time
        and decoded by a resumable inflater as it arrives (_PieceDecompressor).  zdict=: the preset dictionary the
        stream was compressed against (zlib.compressobj(zdict=...)); flate and zlib only, gzip raises ValueError."""
        zdict = _zdict_for(self._container, zdict)  # (gzip: ValueError, before an engine is made)
        if piece is None:
            return _Decompressor(self._container, reader, engine, zdict=zdict)
        return _PieceDecompressor(self._container, reader, engine, piece=piece, zdict=zdict)

    Decompressor = decompressor

    def decompress_members(self, data, engine=None):
        """Every concatenated member of `data` (bytes-like, or a reader that is read to its end) in one GPU call
        (flate_hip_decompress_members): the bytes a caller collects who decodes member by member with decompressor() and
        reset().  Raises the error of the first member that fails, as that loop would."""
        eng = engine or default_engine()
        data = _read_all(data)
        cap = max(1 << 16, len(data) * 64)
        while True:
            outs, st, _, _ = eng.decompress_members([data], self._container, 0, caps=[cap])
            if st[0] == 100 and cap < (1 << 34):
                cap *= 8
                continue
            break
        raise_for_status(st[0])
        return outs[0]

    def build_index(self, data, spacing=None, engine=None):
        """A seek index over the first member of `data` (bytes-like, or a reader that is read to its end): the stream is
        decoded once (flate_hip_index_build) and every `spacing` output bytes or so (default 1 MiB) a block start is kept
        with the 32 KiB in front of it; StreamIndex.read_at then decodes only from the nearest point.  Raises the stream's
        error if it does not decode."""
        eng = engine or default_engine()
        data = _read_all(data)
        ix, _, st, _ = eng.build_index([data], self._container, 0, spacing)
        raise_for_status(st[0])
        return StreamIndex(ix)

    def scan_index(self, data, spacing=None, engine=None):
        """A window-free seek index over the first member of `data` (bytes-like, or a reader that is read to its end),
        made without decoding it (flate_hip_index_scan): a stream written with full flushes (pigz -i, Z_FULL_FLUSH) has a
        point at every flush the spacing rule keeps (default 1 MiB) behind which no match reaches in front of it; any
        other stream has point 0 alone.  The footer is not compared.  Raises the stream's error if the size probe
        reports one."""
        eng = engine or default_engine()
        data = _read_all(data)
        ix, _, st, _ = eng.scan_index([data], self._container, 0, spacing)
        raise_for_status(st[0])
        return StreamIndex(ix)

    def index_from_bytes(self, blob, data, engine=None):
        """the StreamIndex of StreamIndex.to_bytes() and the stream it was built from"""
        return StreamIndex.from_bytes(blob, data, engine)


class StreamIndex:
    """Random access into one compressed stream (ContainerModule.build_index).  There is no checksum over a part of a
    stream: the index must be used with the bytes it was built from."""

    def __init__(self, index):
        self._ix = index
        self.size = index.info(0)[0]

    @classmethod
    def from_bytes(cls, blob, data, engine=None):
        eng = engine or default_engine()
        ix = eng.index_from_bytes(blob, [_read_all(data)])
        if ix.n != 1 or ix.info(0)[1] != 0:
            raise ValueError("not the index of one stream that decoded")
        return cls(ix)

    def points(self):
        """[(in_bit, out_pos)]: where decoding can start"""
        return self._ix.points(0)

    def read_ranges(self, ranges):
        """[(offset, n)] -> list of bytes, each clipped to the stream's size"""
        outs, st = self._ix.read_ranges([(0, int(o), int(n)) for o, n in ranges])
        for s in st:
            raise_for_status(s)
        return outs

    def read_at(self, offset, n):
        return self.read_ranges([(offset, n)])[0]

    def to_bytes(self):
        return self._ix.to_bytes()

    def close(self):
        self._ix.close()


def compress_bytes(data, container=_capi.RAW, mode=6, engine=None):
    w = io.BytesIO()
    c = _Compressor(container, mode, w, engine)
    c.compress(data)
    c.finish()
    return w.getvalue()
