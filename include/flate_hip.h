/*
 * flate_hip.h -- C ABI of libflate_hip.so: the MI355X (gfx950) DEFLATE engine that
 * stands behind ianic/flate's compress / decompress / compressor / decompressor
 * API (reference: /root/reference/src/flate.zig:9-71, src/gzip.zig:4-66,
 * src/zlib.zig:4-66).
 *
 * The boundary is batch-shaped: one call processes n independent chunks
 * ("chunk" = one complete deflate/gzip/zlib stream, i.e. what one
 * `compress(reader, writer, options)` call of the reference produces, or what
 * one `decompress(reader, writer)` call consumes).  Plain pointers and sizes
 * only; no torch / HIP types in the signatures (hipStream_t travels as void*).
 *
 * What each entry point replaces in the reference:
 *   flate_hip_compress_batch    deflate.compress            deflate.zig:56-60
 *                               (= compressor + compress + finish, :138,304,344)
 *                               deflate.huffman.compress    deflate.zig:402-406
 *                               deflate.store.compress      deflate.zig:421-425
 *                               via flate.zig:28-30,44-47,59-62 and the gzip /
 *                               zlib twins (gzip.zig:23-25, zlib.zig:23-25)
 *   flate_hip_compress_flush    Compressor.write / flush / finish with LZ history kept
 *                               across flushes              deflate.zig:335-337, 344-347,
 *                               363-367 (sync flush: 00 00 ff ff, :276-278)
 *   flate_hip_decompress_batch  inflate.decompress          inflate.zig:14-17
 *                               via flate.zig:10-12, gzip.zig:5-7, zlib.zig:5-7
 *   flate_hip_compress_bound    (no reference twin: the Zig writer grows)
 *   status codes                the reference's error set, 1:1
 *                               (bit_reader.zig:29, container.zig:45-51,
 *                               huffman_decoder.zig:35-40, inflate.zig:72-78)
 *
 * All work runs on the GPU.  There is no CPU fallback: if no HIP device is
 * usable every call fails with FLATE_HIP_E_NO_DEVICE.
 */
#ifndef FLATE_HIP_H
#define FLATE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct flate_hip_ctx* flate_hip_handle;
typedef struct flate_hip_plan* flate_hip_plan_t;

/* container tag -- container.zig:18-21 */
enum { FLATE_HIP_RAW = 0, FLATE_HIP_GZIP = 1, FLATE_HIP_ZLIB = 2 };

/* mode: 0 = store-only (deflate.zig:420-434), 1 = huffman-only (:401-415),
 * 4..9 = Level.level_4 .. level_9 (:23-32; fast=4, default=6, best=9). */
enum { FLATE_HIP_MODE_STORE = 0, FLATE_HIP_MODE_HUFFMAN = 1, FLATE_HIP_MODE_DEFAULT = 6 };

/* where in / out / offsets / lengths / status live */
enum { FLATE_HIP_MEM_HOST = 0, FLATE_HIP_MEM_DEVICE = 1 };

/* call-level return codes */
enum {
    FLATE_HIP_OK = 0,
    FLATE_HIP_E_NO_DEVICE = -1,   /* no usable HIP device / kernel image */
    FLATE_HIP_E_INVALID_ARG = -2,
    FLATE_HIP_E_ALLOC = -3,       /* workspace allocation failed */
    FLATE_HIP_E_LAUNCH = -4,      /* a HIP call failed; see flate_hip_last_error */
    FLATE_HIP_E_UNSUPPORTED = -5  /* reserved */
};

/* per-chunk status: the reference's error names, same numbering as the oracle */
enum {
    FLATE_HIP_ST_OK = 0,
    FLATE_HIP_ST_END_OF_STREAM = 1,
    FLATE_HIP_ST_BAD_GZIP_HEADER = 2,
    FLATE_HIP_ST_BAD_ZLIB_HEADER = 3,
    FLATE_HIP_ST_WRONG_GZIP_CHECKSUM = 4,
    FLATE_HIP_ST_WRONG_GZIP_SIZE = 5,
    FLATE_HIP_ST_WRONG_ZLIB_CHECKSUM = 6,
    FLATE_HIP_ST_INVALID_CODE = 7,
    FLATE_HIP_ST_OVERSUBSCRIBED_HUFFMAN_TREE = 8,
    FLATE_HIP_ST_INCOMPLETE_HUFFMAN_TREE = 9,
    FLATE_HIP_ST_MISSING_END_OF_BLOCK_CODE = 10,
    FLATE_HIP_ST_INVALID_MATCH = 11,
    FLATE_HIP_ST_INVALID_BLOCK_TYPE = 12,
    FLATE_HIP_ST_WRONG_STORED_BLOCK_NLEN = 13,
    FLATE_HIP_ST_INVALID_DYNAMIC_BLOCK_HEADER = 14,
    FLATE_HIP_ST_OUTPUT_TOO_SMALL = 100,
    FLATE_HIP_ST_CHUNK_TOO_LARGE = 101, /* reserved; not produced any more: long inputs take the whole-stream path */
    /* Compress, levels 4..9, informational: out / out_len hold exactly the reference's bytes for this input, and those
     * bytes DO NOT inflate to the input.  The reference hands its block writer a full block of 32768 tokens before its
     * window has advanced over the last token's match (deflate.zig:227-230 -> 268-270 -> SlidingWindow.zig:119-123; the
     * advance is at deflate.zig:193), so the raw slice of that block ends up to 258 bytes early and the next block's slice
     * starts there; when exactly ONE of the two blocks goes out stored (block_writer.zig:369) the stream loses those bytes
     * (the first block stored) or holds them twice (the second).  Every inflater -- the reference's included -- then
     * reports a wrong checksum / size for gzip and zlib, and returns other bytes than went in for a raw stream.
     * See FLATE_HIP_DEFLATE_REPAIR_Q1. */
    FLATE_HIP_ST_REFERENCE_Q1_STREAM = 102,
    /* 103 is taken host-side (InvalidState of the Python mirror) */
    FLATE_HIP_ST_NEED_INPUT = 104,  /* inflater feed: all input absorbed, the member is not finished, more input may follow */
    FLATE_HIP_ST_NEED_OUTPUT = 105, /* inflater feed: the output slot is full; feed the unabsorbed rest again with room */
    /* inflate with preset dictionaries (flate_hip_decompress_batch_dict, flate_hip_inflater_set_dictionary) */
    FLATE_HIP_ST_NEED_DICT = 106,   /* a zlib stream with FDICT set, and the stream was given no dictionary */
    FLATE_HIP_ST_WRONG_DICT = 107   /* ... its DICTID is not the Adler-32 of the dictionary the stream was given */
};

/* handle flags (flate_hip_set_flags).  bit0: compress at levels 4..9 hands every block the bytes its tokens cover -- the
 * reference with its window advanced before the tokens are flushed.  Streams differ from the reference's ONLY for inputs on
 * which a full token block ends in a match (the slices that decide "stored or Huffman" move by the match's length); they
 * always inflate to the input and status FLATE_HIP_ST_REFERENCE_Q1_STREAM is never produced.  Default 0: the reference's
 * bytes, whatever they decode to. */
enum { FLATE_HIP_DEFLATE_REPAIR_Q1 = 1 };
int flate_hip_set_flags(flate_hip_handle h, uint32_t flags);

/* decompress flags.  bit0: reference-strict dynamic block header (quirk Q6,
 * inflate.zig:161-180: a code-length repeat that crosses the HLIT/HDIST
 * boundary is rejected, although RFC 1951 3.2.7 allows it and the reference's
 * own encoder emits it).  Default 0: such a header is accepted when valid. */
enum { FLATE_HIP_INFLATE_STRICT_Q6 = 1 };

/* Levels 4..9: an input of up to this many bytes never slides the reference's window and takes
 * the batched chunk path (one workgroup per input); a longer one is compressed as ONE stream by
 * the whole-stream path, byte-identical to Deflate.compress over the whole input
 * (deflate.zig:304-321 with SlidingWindow.zig:36-44, Lookup.zig:43-51).  One level-4..9 input may be
 * at most 0xfff00000 bytes (stream positions are 32-bit); other modes 0xfffffff0. */
#define FLATE_HIP_MAX_LZ_CHUNK 65535u

int flate_hip_create(int device, flate_hip_handle* h);
int flate_hip_destroy(flate_hip_handle h);

/* run on this hipStream_t (NULL = the handle's own stream).  All calls are
 * synchronous on return for FLATE_HIP_MEM_HOST; for FLATE_HIP_MEM_DEVICE the
 * work is enqueued on the stream and the call returns without a device sync
 * unless flate_hip_set_sync(h, 1) (default 1). */
int flate_hip_set_stream(flate_hip_handle h, void* hip_stream);
int flate_hip_set_sync(flate_hip_handle h, int sync_on_return);

/* upper bound of one chunk's output for n input bytes */
size_t flate_hip_compress_bound(size_t n, int container, int mode);

/*
 * Compress n_chunks independent chunks.
 *   in       all input bytes; chunk i is in[in_off[i] .. in_off[i+1])
 *   in_off   n_chunks+1 offsets (bytes)
 *   out      output buffer; chunk i owns the slot out[out_off[i] .. out_off[i+1])
 *   out_off  n_chunks+1 slot starts (bytes), ascending; the slots must not
 *            overlap and `out` must be 4-byte aligned
 *   out_len  n_chunks produced lengths (bytes)
 *   status   n_chunks FLATE_HIP_ST_* codes
 * The bytes of chunk i are exactly what the reference writes for the same
 * input with the same container and level/mode (status 0, or 102 where the reference's own stream is
 * broken: FLATE_HIP_ST_REFERENCE_Q1_STREAM).
 * Host buffers (FLATE_HIP_MEM_HOST): a slot's bytes beyond out_len[i] are unspecified (zeros or
 * what the caller had there; a pinned `out` is written in place by the DMA engine and a kernel).
 */
int flate_hip_compress_batch(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off,
                             uint32_t n_chunks, int container, int mode, uint8_t* out,
                             const uint64_t* out_off, uint64_t* out_len, int32_t* status,
                             int memkind);

/*
 * Asynchronous device batches.  flate_hip_compress_batch(MEM_DEVICE) has to read the offset arrays
 * back and build its chunk / block tables on the host before it can launch (two short blocking
 * copies per call).  A caller whose batch layout repeats -- the same chunk sizes and output slots call
 * after call, as in a pipeline that compresses batch k + 1 while batch k's output is on the wire --
 * plans it once from HOST copies of the offsets; flate_hip_compress_planned then only enqueues kernels on
 * the handle's stream (no allocation, no copy from or to the host, no wait; with set_sync(0) it returns
 * at once).  Inputs of more than 65535 bytes at levels 4..9 (the whole-stream path) are not plannable:
 * FLATE_HIP_E_UNSUPPORTED.  Same output bytes as flate_hip_compress_batch.
 */
int flate_hip_plan_compress(flate_hip_handle h, const uint64_t* in_off_host, const uint64_t* out_off_host,
                            uint32_t n_chunks, int container, int mode, flate_hip_plan_t* plan);
int flate_hip_compress_planned(flate_hip_handle h, flate_hip_plan_t plan, const uint8_t* in, uint8_t* out,
                               uint64_t* out_len, int32_t* status);
int flate_hip_plan_destroy(flate_hip_handle h, flate_hip_plan_t plan);

/*
 * One stream with sync-flush points (levels 4..9, huffman-only, store-only): what a Compressor
 * / SimpleCompressor of the reference (deflate.zig:335-337, 474-478) has
 * written after   write(in[0 .. p0]); flush(); write(in[p0 .. p1]); flush(); ...   and, when
 * `finish` is non-zero, write(rest); finish().  flush_pos: n_flush ascending stream positions
 * (<= n; equal neighbours = flush called twice).  Without `finish` the last flush point must be
 * n and the output ends with that flush's marker.  Output of a shorter prefix of the same call
 * sequence is a prefix of this output, so a streaming wrapper emits only what is new.
 * The LZ77 history survives a flush (deflate.zig:335-337): matches reach back across it, but
 * never run over it.  Host buffers only (memkind FLATE_HIP_MEM_HOST).
 */
int flate_hip_compress_flush(flate_hip_handle h, const uint8_t* in, uint64_t n, const uint64_t* flush_pos,
                             uint32_t n_flush, int finish, int container, int mode, uint8_t* out,
                             uint64_t out_cap, uint64_t* out_len, int32_t* status, int memkind);

/*
 * Decompress n_chunks independent streams (same argument shape).  out_len[i] is the
 * number of bytes produced; status[i] the reference's error name for a bad stream.
 * consumed (optional, may be NULL) receives the input bytes used by each stream, so a
 * caller can walk concatenated members the way Inflate.reset() does (inflate.zig:301-309).
 * Stream order: the call always waits once for the offsets; beyond that a batch of short streams is
 * only enqueued (set_sync(0)).  A batch with long streams (>= 128 KiB, at most 140 of them) is cut
 * into spans and BLOCKS ON THE HOST three to four times between its kernels (the chain of spans is
 * followed on the CPU): such a call cannot be captured in a graph or overlapped behind other work on the
 * stream.  FLATE_HIP_INFLATE_SPANS=0 (environment) or flag bit 0 keeps the old one-workgroup-per-stream path.
 * Host buffers (FLATE_HIP_MEM_HOST): a slot's bytes beyond out_len[i] may be overwritten with zeros.
 */
int flate_hip_decompress_batch(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off,
                               uint32_t n_chunks, int container, int flags, uint8_t* out,
                               const uint64_t* out_off, uint64_t* out_len, int32_t* status,
                               uint64_t* consumed, int memkind);

/*
 * Decompress n_chunks independent streams that were compressed against preset dictionaries (zlib's deflateSetDictionary,
 * Python's zlib.compressobj(zdict=...)).  The first twelve arguments are those of flate_hip_decompress_batch, and so are
 * out_len, consumed, the footer check and the rules for the slots.  Then:
 *   dict      all dictionary bytes; dictionary d is dict[dict_off[d] .. dict_off[d+1]), of any length, 0 included
 *   dict_off  n_dicts + 1 ascending offsets
 *   n_dicts   number of dictionaries (0: dict and dict_off may be NULL, and every dict_of entry is 0xffffffff)
 *   dict_of   n_chunks entries: the dictionary of stream i, or 0xffffffff for a stream without one.  NULL is allowed only
 *             with n_dicts == 1: every stream uses dictionary 0.
 * All arrays live where memkind says; dict_off and dict_of are read back once, as the other offsets are.
 * Only the last 32768 bytes of a dictionary are history; its Adler-32 covers all of it.
 *   raw (container 0)    the stream's dictionary is its history from the first byte.
 *   zlib (container 2)   FDICT set: the four big-endian bytes behind the header (DICTID, RFC 1950 2.2) must be the
 *                        Adler-32 of the stream's dictionary, else FLATE_HIP_ST_WRONG_DICT; a stream without a dictionary
 *                        is FLATE_HIP_ST_NEED_DICT; a stream that ends inside DICTID is EndOfStream.  consumed counts the
 *                        four bytes.  FDICT clear: the dictionary is NOT used and the stream decodes exactly as
 *                        flate_hip_decompress_batch decodes it (zlib.decompressobj(15, zdict) does the same).
 *   gzip                 has no dictionaries: FLATE_HIP_E_INVALID_ARG.
 * InvalidMatch is a distance beyond (bytes produced so far + min(dictionary length, 32768)).  The footer's Adler-32 is over
 * the output alone.
 * Every stream of such a call is decoded by the wave-per-stream kernel: there are no spans and no workgroup-per-stream
 * kernel here, so a LONG stream with a dictionary runs at the speed of one wave.  The shape this call is made for is a
 * large batch of short records that share a few dictionaries.  The Adler-32 of every dictionary is computed once per call.
 * Not covered: the size probe, flate_hip_decompress_members, the sharded entry points.  (Compressing with a dictionary:
 * flate_hip_compress_batch_dict, below.)
 * flate_hip_decompress_batch itself is unchanged: it knows nothing of FDICT.
 */
int flate_hip_decompress_batch_dict(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks,
                                    int container, int flags, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                                    int32_t* status, uint64_t* consumed, int memkind, const uint8_t* dict,
                                    const uint64_t* dict_off, uint32_t n_dicts, const uint32_t* dict_of);

/*
 * Compress n_chunks independent records against preset dictionaries, levels 4..9: the streams that
 * flate_hip_decompress_batch_dict (and zlib.decompressobj(wbits, zdict=...)) inflate.  The first eleven arguments are
 * those of flate_hip_compress_batch, the four dictionary arguments exactly those of flate_hip_decompress_batch_dict (any
 * dictionary length, 0 included; dict_of[i] == 0xffffffff: no dictionary; dict_of == NULL only with n_dicts == 1; all
 * arrays live where memkind says; dict_off and dict_of are read back once, as the other offsets are).
 *
 * What "compressed against a dictionary" means.  The reference has no dictionaries, but its Compressor keeps the LZ77
 * history across a sync flush and a flush ends on a byte boundary.  With T the last min(length, 32768) bytes of the
 * dictionary and R the record: a raw-container reference compressor does  write(T); flush();  -- L bytes so far, ending
 * in 00 00 ff ff --  write(R); finish();  and the stream of R is its output FROM BYTE L ON.
 *   raw (container 0)    that stream.
 *   zlib (container 2)   78 bb (the reference's 78 9c with FDICT set and FCHECK made good), DICTID = the Adler-32 of
 *                        the WHOLE dictionary, big endian, that stream, the big-endian Adler-32 of R alone.
 *   gzip                 has no dictionaries: FLATE_HIP_E_INVALID_ARG.  So are modes 0 and 1.
 * A stream without a dictionary: bytes and status exactly those of flate_hip_compress_batch (zlib: 78 9c, no DICTID).
 * A stream with a dictionary, an empty one included (zlib: FDICT set, DICTID 00 00 00 01): status 0, or 100 when the slot is
 * too small; 102 and FLATE_HIP_DEFLATE_REPAIR_Q1 as in flate_hip_compress_batch (a record needs more than 32768
 * tokens for that: next to no history).  flate_hip_compress_bound(n, container, mode) + 4 bytes are always enough.
 * One difference from zlib's deflateSetDictionary: the tokenizer ran dry at the flush, so the last three positions of the
 * dictionary never enter the hash table (zlib inserts them when the record's first bytes arrive).  A match can begin at
 * any other position of T and run on into the record; none begins at its last three.  The streams are valid either way.
 * Limit: min(dictionary length, 32768) + record length <= 65535 for every stream with a dictionary -- the reference's
 * window never slides on such a stream --, else the whole call returns FLATE_HIP_E_UNSUPPORTED and writes nothing.
 * n_chunks == 0: FLATE_HIP_OK.
 * The dictionary costs a record a copy, not a parse: history and record are written side by side into a workspace of the
 * handle (bounded per pass: at most 2048 such streams at a time, however many the call has), the tokenizer's targets
 * begin behind the history, and nothing is emitted for it.  The Adler-32 of every dictionary is computed once per call.
 * Waits: the call reads its offset arrays and dict_of back first, and the host waits for the stream several times per
 * pass (the tables of a whole-stream pass, the tokenizer's verdict).  It cannot be captured in a graph, as is true of
 * any whole-stream pass.
 * Not covered: records beyond the limit, the resumable deflater, flate_hip_compress_flush with a dictionary, planned and
 * sharded calls, sharing one dictionary's hash chains between records (every stream builds the chains of its own copy).
 */
int flate_hip_compress_batch_dict(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks,
                                  int container, int mode, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                                  int32_t* status, int memkind, const uint8_t* dict, const uint64_t* dict_off,
                                  uint32_t n_dicts, const uint32_t* dict_of);

/*
 * Joined compress, levels 4..9: every input becomes ONE valid gzip / zlib / raw stream made of independent pieces, at the
 * rate of the batched chunk path -- what pigz -i and zlib's Z_FULL_FLUSH give.  The argument shape, the memory kinds and
 * the rules for the slots are those of flate_hip_compress_batch (stream i is in[in_off[i] .. in_off[i+1]), its slot
 * out[out_off[i] .. out_off[i+1])); piece_bytes is 1..65535, 0 means 65535.
 *   pieces   stream i has N bytes and P = max(1, ceil(N / piece_bytes)) pieces; piece k is its bytes
 *            [k * piece_bytes, min((k + 1) * piece_bytes, N)).  Every piece is compressed with no history.
 *   bytes    the container's header, F(piece_0) .. F(piece_{P-2}), L(piece_{P-1}), the container's footer, where
 *            L(x) is what flate_hip_compress_batch writes for x as a raw stream, and
 *            F(x) is what a fresh raw reference compressor has written after write(x); flush() (deflate.zig:335-337,
 *            276-278): L(x) with the final-block bit of its last block cleared, then the sync-flush marker -- 00 00 ff ff
 *            when 1..5 padding bits stand in the last byte of that block, 00 00 00 ff ff when it ends 0, 6 or 7 bits into
 *            a byte (a stored block ends at 0).
 *            The footer covers the WHOLE stream: gzip CRC-32 and ISIZE = N mod 2^32, zlib the big-endian Adler-32.
 *            With P == 1 the stream is byte for byte that of flate_hip_compress_batch with the same container.
 *            N may exceed 4 GiB: a joined stream has no 32-bit stream positions.
 *   status   0; FLATE_HIP_ST_OUTPUT_TOO_SMALL (100) when the slot is too small -- only that stream is affected, nothing is
 *            written into its slot and out_len is 0 --; FLATE_HIP_ST_REFERENCE_Q1_STREAM (102) when any piece is such a
 *            stream: the bytes are still as defined above (the first non-zero piece status is reported).  With
 *            FLATE_HIP_DEFLATE_REPAIR_Q1 on the handle every piece is repaired and 102 does not occur.
 *   bound    flate_hip_joined_bound(N, piece_bytes, container, mode) = header + the sum over the pieces of
 *            (flate_hip_compress_bound(length, FLATE_HIP_RAW, mode) + 5) + footer always suffices.
 * Modes 0 and 1, a container outside 0..2 or piece_bytes above 65535: FLATE_HIP_E_INVALID_ARG, nothing is written.
 * n_streams == 0: FLATE_HIP_OK.  A call may have at most 2^31 - 1 pieces, else FLATE_HIP_E_UNSUPPORTED.
 * What it costs in ratio: no match reaches back over a piece's start and every piece has its own Huffman tables
 * (DESIGN.md 4b'''': 256 MiB of text at level 6, 65535-byte pieces against the whole-stream path).
 * How: the pieces go through the chunk passes of flate_hip_compress_batch as raw chunks (no kernel of those changes);
 * behind every pass k_join_open clears the final-block bits and writes the markers while the pass's block plans are
 * valid, and k_checksum takes the container's checksum a piece at a time; then k_join_scan gives every piece its place
 * (a scan of the piece lengths per stream) and combines the pieces' checksums on the device, and k_join_pack copies the
 * pieces behind the header (16-byte stores) and writes header and footer.  No byte outside a stream's slot is written.
 * Workspace: the pieces are compressed into a scratch region of the handle that holds ALL pieces of the call -- the
 * simple call-wide layout, not a per-pass one: per piece its raw bound + 5 rounded up to 16 bytes with 16 to spare (about
 * 1.02 x the input + 170 bytes a piece) and 36 bytes of tables, besides the workspace of a chunk-path pass;
 * flate_hip_debug_workspace_bytes counts it.
 * Waits: those of a chunk-path batch on the same memory kind -- the offsets are read back once, and the host waits once per
 * pass for the pass's tables -- and one more for the call's own tables.  Not capturable in a graph.
 * FLATE_HIP_MEM_HOST: input and slots are staged whole (no pinned sub-batch pipeline); a slot's bytes beyond out_len[i]
 * are unspecified.
 * Not covered: planned, sharded and dictionary calls, pieces above 65535 bytes or pieces that keep history, the resumable
 * deflater.
 */
size_t flate_hip_joined_bound(uint64_t n, uint32_t piece_bytes, int container, int mode);
int flate_hip_compress_joined(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams,
                              uint32_t piece_bytes, int container, int mode, uint8_t* out, const uint64_t* out_off,
                              uint64_t* out_len, int32_t* status, int memkind);

/*
 * Size probe: how many bytes each of n_chunks independent streams inflates to, without inflating it.  The arguments have
 * the shape of flate_hip_decompress_batch without `out` and `out_off`; flags bit 0 = FLATE_HIP_INFLATE_STRICT_Q6;
 * consumed may be NULL.
 *   status[i]    what flate_hip_decompress_batch reports for stream i with a slot that is large enough, with one
 *                exception: the footer is read but not compared (there are no bytes to sum).  A truncated footer is
 *                still EndOfStream; where decompress would report WrongGzipChecksum, WrongGzipSize or WrongZlibChecksum
 *                the probe reports 0.  OutputTooSmall never occurs.  InvalidMatch is exact: a distance beyond the bytes
 *                produced so far is refused, as are a length or distance out of range.
 *   sizes[i]     status[i] == 0: exactly the out_len[i] decompress would produce (64-bit: a stream's output may exceed
 *                4 GiB).  status[i] != 0: unspecified.
 *   consumed[i]  as for decompress: header, blocks and footer of the first member, trailing bytes not counted, so a
 *                caller can walk concatenated members.
 * Nothing is written anywhere except sizes, status and consumed.  The handle's workspace does not grow with the output:
 * per stream it holds the chunk table entry and, for a long stream, its scan points and span records.
 * FLATE_HIP_MEM_HOST: the input is staged and the call is synchronous.  FLATE_HIP_MEM_DEVICE: all arrays are device
 * memory; the offsets are read back once, as decompress does.  A batch without a stream that is cut only enqueues its
 * kernel on the handle's stream and flate_hip_set_sync decides about the final wait.  Long streams (at least
 * FLATE_HIP_INFLATE_SPANS bytes, 128 KiB by default; at most 256 of them, in a batch with no more long streams than the
 * device has CUs; never with flag bit 0) are cut at block starts and counted by many waves at once: such a call WAITS
 * ON THE HOST twice (for the block starts found, for the span records, whose chain is followed on the CPU) and once
 * more for the results it writes itself.  A stream whose chain does not close is counted whole by one wave: always
 * correct, only slow.  n_chunks == 0 returns FLATE_HIP_OK; argument errors as for decompress.  The counters of
 * flate_hip_debug_inflate_paths are left untouched.
 */
int flate_hip_decompressed_sizes(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks,
                                 int container, int flags, uint64_t* sizes, int32_t* status, uint64_t* consumed,
                                 int memkind);

/*
 * Every member of concatenated gzip / zlib / raw streams, in one call.  The arguments have the shape of
 * flate_hip_decompress_batch; consumed and n_members may be NULL.  The meaning is exactly the loop a caller of
 * flate_hip_decompress_batch writes: for stream i with bytes S = in[in_off[i] .. in_off[i+1]) and slot O,
 *
 *     pos = 0; produced = 0; members = 0
 *     repeat
 *         decode ONE member from S[pos:] into O[produced:]   (what flate_hip_decompress_batch does, same flags)
 *         if its status != 0: status[i] = that status; stop
 *         produced += its out_len; pos += its consumed; members += 1
 *     until pos == len(S)
 *     status[i] = 0
 *
 * and out_len[i] = produced, consumed[i] = pos, n_members[i] = members: all three count only the members in front of
 * the first failing one, whose bytes are in the slot; slot bytes beyond out_len[i] are unspecified.  The first member is
 * always attempted, so an empty stream is EndOfStream (1) in all three containers.  Trailing bytes are a further member:
 * behind a gzip member they give BadGzipHeader (2) when 10 or more are left and the magic or the method is wrong,
 * EndOfStream (1) when fewer than 10 are left.  A member that does not fit the rest of the slot gives
 * FLATE_HIP_ST_OUTPUT_TOO_SMALL (100) for the stream.  A stream may be at most 0xfffffff0 bytes; n_streams == 0 returns
 * FLATE_HIP_OK.  flate_hip_debug_inflate_paths afterwards describes the decode of the members.
 *
 * How the members are found.  gzip: every position of 1f 8b 08 inside a stream is a candidate, every candidate is probed
 * as flate_hip_decompressed_sizes probes a stream (a wave each, no output), and each stream's chain of candidates is
 * followed on the device from its first byte; a candidate no chain reaches -- the magic inside compressed bits, a stored
 * block, a file name -- costs its probe and nothing else.  zlib and raw members cannot be told from their bytes; their
 * streams are walked member by member by one wave each, and so are gzip streams when FLATE_HIP_MEMBER_SCAN=0 or when a
 * call has more candidates than FLATE_HIP_MEMBER_CANDIDATES (4194304 by default).  The walk is always correct, only slow:
 * one long file is walked by one wave.  A long member is likewise counted by one wave before it is decoded.  The members
 * are then decoded as a batch of their own by the kernels of flate_hip_decompress_batch (long members by spans or a
 * workgroup each), which compare the footers; the probe does not.  The walk's member table takes 12 bytes for every 20
 * (gzip), 8 (zlib) or 2 (raw) bytes of input.
 *
 * FLATE_HIP_MEM_HOST: input and slots are staged and the call is synchronous.  FLATE_HIP_MEM_DEVICE: all arrays are device
 * memory.  Either way the call WAITS ON THE HOST three times beyond what the decode of the members waits for as any
 * batch on device memory does: for the offsets, for the number of candidates (walk: of members), and for the member
 * table.  It cannot be captured in a graph.
 */
int flate_hip_decompress_members(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams,
                                 int container, int flags, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                                 int32_t* status, uint64_t* consumed, uint32_t* n_members, int memkind);

/*
 * Random access: a seek index over a batch of streams, and byte ranges of their output decoded from it.
 *
 * A POINT of a stream is a block start with what a decoder needs to begin there: in_bit, the position of the block's
 * BFINAL bit counted from the stream's first byte (container header included); out_pos, the bytes produced before the
 * block; and a window, the min(out_pos, 32768) output bytes in front of out_pos.  Which block starts are points is a
 * rule of the stream and `spacing` (S >= 1; 0 means 1 MiB) alone: the first block is point 0, and block k >= 1 is a point
 * iff the block before it holds a grid line g * S in (pos[k-1], pos[k]].  So out_pos ascends strictly, a stream of N bytes
 * has at most 1 + N / S points, and the end of the last block is no point.  Only the first member of a stream is
 * indexed, as flate_hip_decompress_batch decodes only that.
 *
 * flate_hip_index_build: the first twelve arguments are those of flate_hip_decompress_batch, and out, out_len, status and
 * consumed get exactly what that call writes for them -- it is that call which runs, spans and all.  Then the block
 * starts of every stream whose status is 0 are walked (the size probe's loop: nothing is decoded a second time) and the
 * points' windows are copied out of the decoded bytes into device memory the index owns: 32 KiB a point.  A stream whose
 * status is not 0 (a wrong footer and FLATE_HIP_ST_OUTPUT_TOO_SMALL included) has no points and size 0.  The index
 * remembers container, spacing, n_streams and per stream in_len, size and status.  Short streams are walked by a wave
 * each.  Long streams are cut as flate_hip_decompressed_sizes cuts them (same rule, same FLATE_HIP_INFLATE_SPANS) and
 * walked a wave per span, each span knowing its output base once the spans' chain is followed; the decode path's span
 * inflater does not run a second time.  A stream whose chain does not close is walked whole by one wave: always
 * correct, only slow.  flate_hip_debug_index_paths counts the good streams of the last build that went either way.
 * The call WAITS ON THE HOST as flate_hip_decompress_batch does, then for out_len and status, for the block starts
 * found and the span records (long streams), for the walkers' points, and for the window copies; a host caller's batch
 * is read where that call staged it.  The workspace holds 16 bytes per possible point
 * (1 + out_len / S per stream) besides the decode's.  n_streams == 0 gives an empty index; argument errors as for
 * decompress, and *idx is NULL whenever the return value is not FLATE_HIP_OK.  An error behind the decode -- no memory
 * for the walk or the windows, a failed HIP call, or FLATE_HIP_E_LAUNCH with "disagrees with its decode" in
 * flate_hip_last_error when a walk does not arrive at the size the decode produced (not seen; it would be a fault of the
 * library) -- leaves out, out_len, status and consumed as flate_hip_decompress_batch wrote them, valid, and no index.
 *
 * flate_hip_index_stream_info / flate_hip_index_points: what the index holds for one stream; the arrays are host memory,
 * at most cap entries are written, the return value is the number of points (negative: an error code).
 *
 * flate_hip_index_export / flate_hip_index_import: the index as one self-contained little-endian blob in host memory
 * (layout: INTEGRATION.md), and back, on any handle.  import believes nothing: counts, offsets, order and window lengths
 * are checked against `bytes`, and anything else than a blob export wrote gives FLATE_HIP_E_INVALID_ARG.
 *
 * flate_hip_decompress_ranges: range j asks for bytes [range_begin[j], range_begin[j] + range_len[j]) of the output of
 * stream range_stream[j], clipped to the stream's size: L' = min(len, size - begin), 0 when begin >= size.  Its slot is
 * out[out_off[j] .. out_off[j+1]) (n_ranges + 1 offsets).  n_streams and every in_len must be those of the index
 * (else FLATE_HIP_E_INVALID_ARG), and `in` must hold the bytes the index was built from.
 *   out_len[j] = L', status[j] = 0    the bytes are at the start of the slot
 *   the stream's build status, 0      the stream failed in the build
 *   FLATE_HIP_ST_OUTPUT_TOO_SMALL, 0  the slot is smaller than L'; nothing is written
 *   a decoder status, 0               the bytes no longer decode.  THERE IS NO CHECKSUM TO COMPARE: input that differs
 *                                     from what the index was built from and still decodes gives wrong bytes silently.
 * No byte outside the first out_len[j] bytes of a slot is written.  Each range is decoded by one wave from the last point
 * with out_pos <= begin, with the point's window as history, into scratch of the handle (skip + L' + 258 bytes, skip
 * being begin - out_pos: below S plus the length of the block that holds the grid line, which nothing bounds), and the
 * requested bytes are copied to the slot.  A call runs in passes of at most FLATE_HIP_INDEX_PASS_BYTES of scratch
 * (256 MiB by default; a range that needs more is a pass alone); flate_hip_debug_workspace_bytes counts the scratch and
 * flate_hip_debug_index_passes tells the passes of the last call.  All arrays are where memkind says; the offsets and
 * the three range arrays are read back once, and the job tables are uploaded behind a wait: the call cannot be captured
 * in a graph.  Of a host caller's input only the bytes the decodes can consume are staged (from a range's point to the
 * first point at or behind its end; a stream without a range costs nothing), and the results come home packed.
 * range_stream[j] >= n_streams gives FLATE_HIP_E_INVALID_ARG; n_ranges == 0 returns FLATE_HIP_OK.
 *
 * flate_hip_compress_joined_indexed: the first twelve arguments, the bytes written, out_len, status and the error
 * returns are exactly those of flate_hip_compress_joined -- it is that code which runs -- and *idx gets a FRESH index of
 * the streams just written.  A fresh point is the start of a piece: a byte boundary, with no history in front of it, so
 * a fresh point has an empty window, win_bytes is 0 and the index holds NO device memory: 24 bytes a point on the host.
 * Stream i with status 0 (N bytes in pieces of `piece`): piece k is a candidate with out_pos = k * piece and in_bit =
 * 8 * (the piece's first byte - the stream's first byte), the BFINAL bit of the piece's first block; which candidates
 * are points is the rule above over the piece starts (piece 0; piece k >= 1 iff a grid line lies in ((k-1) * piece,
 * k * piece]; spacing 1: every piece; 0: 1 MiB).  Its record holds in_len = out_len[i], size = N, status 0.  A stream
 * whose status is not 0 (FLATE_HIP_ST_OUTPUT_TOO_SMALL, and 102 without FLATE_HIP_DEFLATE_REPAIR_Q1: a piece of it may
 * not inflate to `piece` bytes) has no points and size 0, as a stream that failed in flate_hip_index_build.  An empty
 * stream has point 0 and size 0.  The call WAITS ON THE HOST for the stream, whatever flate_hip_set_sync says: the
 * places of the point pieces are collected on the device and read back (8 bytes a point, not a piece), and, device
 * memory, out_len and status.  n_streams == 0 gives an empty index; idx == NULL is FLATE_HIP_E_INVALID_ARG; *idx is NULL
 * whenever the return value is not FLATE_HIP_OK.  An error behind the compress -- a failed HIP call of the read-back, or
 * FLATE_HIP_E_UNSUPPORTED for a stream longer than any decompress call takes (0xfffffff0 bytes) -- leaves out, out_len
 * and status as flate_hip_compress_joined wrote them, valid, and no index.
 * destroy, stream_info, points, export_size, export and import mean on a fresh index what they mean on a windowed one;
 * its blob is version 2 (version 1's header and records, no windows), and import picks the parser by the
 * version field.
 *
 * flate_hip_decompress_ranges ON A FRESH INDEX: the clipped range is cut into PARTS at the points: for every point k
 * from the last with out_pos <= begin to the last with out_pos <= begin + L' - 1 the part is [max(begin, pos_k),
 * min(begin + L', pos_k+1 or size)).  Every part is decoded by a wave of its own, with no history.  A part that starts
 * at its point and ends at the next point or at the stream's size is DIRECT: it is decoded straight into the slot, at
 * pos_k - begin, with room for exactly its length; no wave stores outside its own part.  Any other part -- per range
 * at most the first and the last -- goes through scratch (skip + len + 258 bytes) and is copied to the slot.  Passes are
 * cut over the parts' scratch (a direct part costs none); flate_hip_debug_index_parts counts the direct and the scratch
 * parts of the last call.  status[j] is the first non-zero status among the range's parts in stream order, else 0;
 * out_len[j] is L' when the status is 0, else 0.  THE CONTRACT DIFFERS FROM THE ONE ABOVE in one point: no byte outside
 * the first L' bytes of a slot is written, but when status[j] is not 0 those L' bytes are unspecified -- other parts of
 * the range may have landed.  (FLATE_HIP_ST_OUTPUT_TOO_SMALL and a failed stream still write nothing.)  The warning
 * about the missing checksum stands.  The host waits as above; of a host caller's input the bytes from every part's
 * point to the next point are staged.  More than 2^31 - 1 parts in a call give FLATE_HIP_E_UNSUPPORTED.
 * On a windowed index the call runs exactly the code described further up.
 *
 * flate_hip_index_scan: a FRESH index over streams written elsewhere (pigz -i, zlib with Z_FULL_FLUSH), found by walking
 * the streams: nothing is decoded into memory and there is no output buffer.  The first ten arguments are those of
 * flate_hip_decompressed_sizes, and sizes, status and consumed get exactly what that call writes for them -- it is that
 * call which runs first, spans and all: the footer is read but not compared (the statuses decompress gives a wrong
 * CRC-32, Adler-32 or ISIZE read 0 here, and such a stream is indexed), FLATE_HIP_ST_INVALID_MATCH is exact, and nothing
 * is written anywhere else.  Then every stream whose status is 0 is walked once more for its points:
 *   A MARK is a block start whose preceding block is a stored block with LEN 0 and BFINAL 0, the trailer of a sync or
 *   full flush; it lies on a byte boundary.  With pos[0] = 0 for block 0 and the positions of the marks behind it in
 *   stream order, the rule above (S = spacing; 0 means 1 MiB) says which marks are KEPT -- as it does for the piece
 *   starts of flate_hip_compress_joined_indexed.  A kept mark at output position c is FRESH iff no match at a position
 *   p >= c has p - distance < c.  The points are block 0 and the fresh kept marks.  A kept mark that is not fresh is
 *   DROPPED, NOT REPLACED: where the kept mark of a cell is a sync flush, the cell's later full flush is not looked for
 *   (spacing 1 keeps every mark that moves forward).  A stream without fresh marks has point 0 alone; a stream whose
 *   status is not 0 has no points and size 0.
 * *idx is of the kind flate_hip_compress_joined_indexed returns: no windows, no device memory, 24 bytes a point on the
 * host, a version-2 blob; destroy, stream_info, points, export_size, export, import and flate_hip_decompress_ranges (the
 * parts path) take it as they take that one.  Short streams are walked by a wave each, long streams a wave per live span
 * where the probe's chain closes (the span records the probe has just read are used: the spans are not counted a second
 * time; flate_hip_debug_index_paths counts the streams of the last scan that went either way), else whole by one wave.
 * The call WAITS ON THE HOST as flate_hip_decompressed_sizes does, whatever flate_hip_set_sync says, then for the
 * offsets, sizes and status (device memory), for the walkers' records, and -- where the lists have room for more than
 * 4096 entries, behind a kernel that packs what was written -- for the walkers' lists; a host caller's batch is read
 * where the probe staged it.  The workspace holds, besides the probe's, 24 bytes per possible mark: per walk its
 * start, its first mark and 1 + out_len / S marks in cells of their own, but no more marks than its input has room for
 * markers (one per 32 bits); and the packed copy of what was written.
 * n_streams == 0 gives an empty index; idx == NULL is FLATE_HIP_E_INVALID_ARG; other argument errors as for the probe;
 * *idx is NULL whenever the return value is not FLATE_HIP_OK.  An error behind the probe -- no memory for the walk, a
 * failed HIP call, FLATE_HIP_E_UNSUPPORTED for a stream longer than 0xfffffff0 bytes, or FLATE_HIP_E_LAUNCH with
 * "disagrees with its probe" in flate_hip_last_error when a walk contradicts the size the probe counted (not seen; it
 * would be a fault of the library) -- leaves sizes, status and consumed as the probe wrote them, valid, and no index.
 *
 * Not covered by the fresh index: replacing a dropped kept mark by a later fresh one in its cell; fresh points at block
 * starts that follow no marker; an index with some points windowed and some fresh; cutting ranges at the points of a
 * windowed index; planned, sharded and dictionary calls; the resumable deflater; pieces that keep history.
 *
 * Not covered: members behind the first of a concatenated stream (split it with flate_hip_decompress_members first);
 * compressed windows; an index for the resumable inflater or for streams with preset dictionaries; the sharded entry
 * points and planned calls; the span path reading an index it is handed.
 */
typedef struct flate_hip_index* flate_hip_index_t;
int flate_hip_index_build(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams, int container,
                          int flags, uint8_t* out, const uint64_t* out_off, uint64_t* out_len, int32_t* status,
                          uint64_t* consumed, int memkind, uint64_t spacing, flate_hip_index_t* idx);
int flate_hip_index_destroy(flate_hip_handle h, flate_hip_index_t idx);
int flate_hip_index_stream_info(flate_hip_handle h, flate_hip_index_t idx, uint32_t stream, uint64_t* size, int32_t* status,
                                uint64_t* n_points);
int64_t flate_hip_index_points(flate_hip_handle h, flate_hip_index_t idx, uint32_t stream, uint64_t* in_bit, uint64_t* out_pos,
                               uint64_t cap);
int flate_hip_index_export_size(flate_hip_handle h, flate_hip_index_t idx, uint64_t* bytes);
int flate_hip_index_export(flate_hip_handle h, flate_hip_index_t idx, uint8_t* blob_host, uint64_t cap);
int flate_hip_index_import(flate_hip_handle h, const uint8_t* blob_host, uint64_t bytes, flate_hip_index_t* idx);
int flate_hip_decompress_ranges(flate_hip_handle h, flate_hip_index_t idx, const uint8_t* in, const uint64_t* in_off,
                                uint32_t n_streams, uint32_t n_ranges, const uint32_t* range_stream,
                                const uint64_t* range_begin, const uint64_t* range_len, uint8_t* out, const uint64_t* out_off,
                                uint64_t* out_len, int32_t* status, int memkind);
int flate_hip_compress_joined_indexed(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams,
                                      uint32_t piece_bytes, int container, int mode, uint8_t* out, const uint64_t* out_off,
                                      uint64_t* out_len, int32_t* status, int memkind, uint64_t spacing, flate_hip_index_t* idx);
int flate_hip_index_scan(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams, int container,
                         int flags, uint64_t* sizes, int32_t* status, uint64_t* consumed, int memkind, uint64_t spacing,
                         flate_hip_index_t* idx);
int flate_hip_debug_index_parts(flate_hip_handle h, uint64_t counts[2]); /* last ranges call: parts decoded straight into a slot | through scratch */
int flate_hip_debug_index_passes(flate_hip_handle h, uint64_t* passes);
int flate_hip_debug_index_paths(flate_hip_handle h, uint64_t counts[2]);

/*
 * Pack the n_chunks produced streams back to back (device memory only): copies
 * out[out_off[i] .. out_off[i] + out_len[i]) to dst[dst_off[i] ..) with
 * dst_off[i] = sum of out_len[k] for k < i; dst_off has n_chunks + 1 entries (the last
 * one is the packed size).  This is the "reassemble the output bitstream" step that
 * precedes the RCCL all-gather of a sharded job; the Zig writer of the reference does
 * the same thing implicitly by writing streams one after another.
 */
int flate_hip_gather_streams(flate_hip_handle h, const uint8_t* out, const uint64_t* out_off,
                             const uint64_t* out_len, uint32_t n_chunks, uint8_t* dst, uint64_t* dst_off);

/*
 * Multi-GPU (one process per GPU): the caller shards the job's chunks over the ranks
 * (contiguous ranges balanced by bytes; inflate: by ISIZE); each rank hands ITS chunks to these entry
 * points together with an RCCL communicator (ncclComm_t as void*, made by the RCCL of the process --
 * torch.distributed's or the caller's own; the library binds to it at run time, it does not link
 * RCCL).  No collective touches the data path; the exchange is the reassembly of the output:
 *
 * compress: the local chunks are compressed exactly as flate_hip_compress_batch(MEM_DEVICE) does, the
 *   produced streams are packed back to back at gathered + rank * slice_bytes (dst_off: n_chunks + 1
 *   offsets inside the slice, device memory), the packed sizes are all-gathered into sizes[world]
 *   (device memory), and every slice goes to every peer in ONE grouped batch of ncclSend / ncclRecv
 *   (xGMI is point to point: each link carries one peer's shard, no ring).  slice_bytes must bound
 *   every rank's packed shard (e.g. the sum of its compress bounds) and be the same on all ranks.
 *   Every peer is sent the largest packed shard's worth of bytes (the sizes are read on the host once per call), not
 *   the slice's capacity.  Afterwards gathered[r * slice_bytes .. + sizes[r]) is rank r's output on every rank -- what the
 *   reference's writer would hold after compressing the ranks' chunks one after the other.
 * decompress: the local streams are inflated straight into this rank's slice (out_off relative to
 *   the slice), then the slices are exchanged the same way.
 * All device memory; work is enqueued on the handle's stream (set_sync decides about the final wait).
 * The reference has no counterpart: it is single-threaded; these replace the loop a
 * caller would write around compress() / decompress() per file.
 */
int flate_hip_compress_batch_sharded(flate_hip_handle h, void* nccl_comm, int rank, int world,
                                     const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks,
                                     int container, int mode, uint8_t* out, const uint64_t* out_off,
                                     uint64_t* out_len, int32_t* status, uint8_t* gathered,
                                     uint64_t slice_bytes, uint64_t* sizes, uint64_t* dst_off);
int flate_hip_decompress_batch_sharded(flate_hip_handle h, void* nccl_comm, int rank, int world,
                                       const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks,
                                       int container, int flags, uint8_t* gathered, uint64_t slice_bytes,
                                       const uint64_t* out_off, uint64_t* out_len, int32_t* status,
                                       uint64_t* consumed);

/*
 * Resumable inflate: n_streams independent stream decoders whose state stays in device memory between calls
 * (the reference's Decompressor, inflate.zig:43-355, that reads from a reader in bounded memory).  Each stream
 * is fed its compressed bytes piece by piece and hands out output as it is decoded; about 74 KiB of device memory
 * per stream (state, carry, 32 KiB history and the decoder's input and output windows), whatever the length of
 * the stream.  flags bit 0 = FLATE_HIP_INFLATE_STRICT_Q6.
 *
 * One feed, per stream i:
 *   in[in_off[i] .. in_off[i+1])  continues the stream where the previous feed left it; consumed[i] bytes of it
 *                                 were absorbed (never passed again; the rest must be).  All of it is absorbed
 *                                 unless the member ended inside it or the output slot filled.
 *   final[i]                      1 = no input follows this piece (the EndOfStream model of the one-shot path)
 *   out[out_off[i] .. out_off[i+1])  slot for this feed's output; out_len[i] bytes written, the rest of the slot is
 *                                 left as it was.  The output of all feeds,
 *                                 concatenated, is what flate_hip_decompress_batch makes of the concatenated input.
 *   status[i]                     FLATE_HIP_ST_OK (member complete, footer checked), FLATE_HIP_ST_NEED_INPUT,
 *                                 FLATE_HIP_ST_NEED_OUTPUT, or an error 1..14 -- sticky: later feeds return it and
 *                                 absorb nothing.  An error is reported while final[i] = 0 only if no later input
 *                                 could change it.  The feed that reports an error absorbs the input up to the
 *                                 error; bytes an earlier feed absorbed stay absorbed.
 * A complete member produces and absorbs nothing until flate_hip_inflater_reset (trailing bytes belong to the next
 * member).  A stream with an empty piece, final 0 and an empty slot is skipped (its state is untouched).  A slot of
 * 1..257 bytes for a stream that is not skipped is FLATE_HIP_E_INVALID_ARG (host memory: the call; device memory: that
 * stream's status, state untouched); 258 bytes or more always make progress.
 * FLATE_HIP_MEM_HOST: synchronous.  FLATE_HIP_MEM_DEVICE: every array is device memory and the call only enqueues
 * (no host wait, no host read of the offsets); flate_hip_set_sync decides about the final wait.
 * flate_hip_inflater_reset (host array `which`) starts a new member on the listed streams.
 */
/* flate_hip_inflater_create flag (beside FLATE_HIP_INFLATE_STRICT_Q6): a zlib stream with FDICT set on a stream that was
 * given no dictionary reads its DICTID and reports FLATE_HIP_ST_NEED_DICT.  Without the flag such a stream is decoded
 * as it always was: the FDICT bit is ignored and the DICTID bytes are taken for deflate data. */
enum { FLATE_HIP_INFLATER_NEED_DICT = 2 };
typedef struct flate_hip_inflater* flate_hip_inflater_t;
int flate_hip_inflater_create(flate_hip_handle h, uint32_t n_streams, int container, int flags, flate_hip_inflater_t* s);
int flate_hip_inflater_destroy(flate_hip_handle h, flate_hip_inflater_t s);
int flate_hip_inflater_reset(flate_hip_handle h, flate_hip_inflater_t s, const uint32_t* which, uint32_t n_which);
int flate_hip_inflater_feed(flate_hip_handle h, flate_hip_inflater_t s, const uint8_t* in, const uint64_t* in_off,
                            const uint8_t* final_, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                            uint64_t* consumed, int32_t* status, int memkind);
/*
 * Give the listed streams (host array `which`) of a raw or zlib inflater one preset dictionary: dict[0 .. dict_len), in
 * memory of kind memkind, any length.  It is copied in (its last 32768 bytes and its Adler-32 are kept): a host
 * buffer is free on return; a device buffer is read on the handle's stream and is free in stream order (on return when
 * `applied` is given or flate_hip_set_sync is on).  It takes effect only on a stream that has absorbed no input since create or reset (a raw
 * stream that has absorbed nothing but whole blocks without output, ending on a byte boundary, counts as such: it has no
 * history yet, and the dictionary is what it would have been in front of those blocks); any
 * other listed stream is left untouched.  applied (host array of n_which bytes, may be NULL) receives 1 or 0 per listed
 * stream; the call waits when it is given.  Feeding then behaves as flate_hip_decompress_batch_dict does for the
 * concatenated pieces, DICTID may be cut anywhere across feeds, and FLATE_HIP_ST_NEED_DICT / _WRONG_DICT are sticky as the
 * other errors are.  flate_hip_inflater_reset drops the dictionary.  A gzip inflater: FLATE_HIP_E_INVALID_ARG.
 */
int flate_hip_inflater_set_dictionary(flate_hip_handle h, flate_hip_inflater_t s, const uint32_t* which, uint32_t n_which,
                                      const uint8_t* dict, uint64_t dict_len, int memkind, uint8_t* applied);

/*
 * Resumable compress: n_streams independent huffman-only (mode 1) or store-only (mode 0) compressors whose state stays
 * in device memory between calls -- the reference's SimpleCompressor (deflate.zig:449-529) written to piece by piece.
 * Levels 4..9 are not resumable yet: flate_hip_deflater_create returns FLATE_HIP_E_UNSUPPORTED for them.  `flags`: 0 or
 * FLATE_HIP_DEFLATE_REPAIR_Q1, which has no effect in modes 0 and 1 (Q1 is a seam between token blocks); other bits
 * are FLATE_HIP_E_INVALID_ARG.
 *
 * One feed, per stream i, with op[i] one of FLATE_HIP_FEED_*:
 *   in[in_off[i] .. in_off[i+1])  the stream's next piece (at most 0xffef0000 bytes), written to the compressor
 *   op[i]                         MORE: write(piece); FLUSH: write(piece) then flush(); FINISH: write(piece) then finish()
 *   out[out_off[i] .. out_off[i+1])  slot for this feed's output (any size, 0 included); out_len[i] bytes written
 *   consumed[i]                   the piece's length (taken whole) or 0 (not taken: send it and its op again)
 *   status[i]                     FLATE_HIP_ST_NEED_INPUT (everything delivered, more may be written),
 *                                 FLATE_HIP_ST_NEED_OUTPUT (output is still pending after this feed), or, after FINISH
 *                                 with everything delivered, the status flate_hip_compress_batch reports for the whole
 *                                 input (0).
 * A feed takes no input from a stream that still has output from an earlier feed: it only hands that output into the
 * slot (consumed 0), and reports NEED_INPUT or the final status once nothing is left.  The output of all feeds from create / reset to FINISH, concatenated, does not depend on how the input was cut:
 * with no FLUSH it is flate_hip_compress_batch of the whole input, with FLUSH feeds flate_hip_compress_flush with flush
 * points at the ends of those feeds -- and streams may be longer than 4 GiB (ISIZE is the length mod 2^32).  After a
 * MORE feed every complete 65535-byte block has been handed out but the last partial byte; after a FLUSH feed
 * everything up to the flush's marker.  A finished stream takes nothing and reports its final status until reset.  A
 * stream with an empty piece, op MORE and an empty slot is skipped (state untouched).
 * Memory: per stream 64 KiB of buffer and 24 bytes of state (carry bits, running checksum, 64-bit total) on the device,
 * whatever the stream's length; a feed's workspace is about 2.1 x the bytes fed plus 64 KiB per stream fed, and output
 * that did not fit a slot is kept (at most one feed's output per stream).  flate_hip_debug_device_bytes reports what
 * the handle's deflaters hold.
 * FLATE_HIP_MEM_HOST: synchronous.  FLATE_HIP_MEM_DEVICE: every array is device memory; the feed reads the offsets and
 * ops back to the host, builds its block tables there and waits for the kernels (not capturable in a graph).
 * flate_hip_deflater_reset (host array `which`) starts a new stream (a new gzip / zlib member) on the listed streams.
 */
typedef struct flate_hip_deflater* flate_hip_deflater_t;
enum { FLATE_HIP_FEED_MORE = 0, FLATE_HIP_FEED_FLUSH = 1, FLATE_HIP_FEED_FINISH = 2 };
int flate_hip_deflater_create(flate_hip_handle h, uint32_t n_streams, int container, int mode, uint32_t flags,
                              flate_hip_deflater_t* d);
int flate_hip_deflater_destroy(flate_hip_handle h, flate_hip_deflater_t d);
int flate_hip_deflater_reset(flate_hip_handle h, flate_hip_deflater_t d, const uint32_t* which, uint32_t n_which);
int flate_hip_deflater_feed(flate_hip_handle h, flate_hip_deflater_t d, const uint8_t* in, const uint64_t* in_off,
                            const uint8_t* op, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                            uint64_t* consumed, int32_t* status, int memkind);
/* test seam: device bytes the handle's deflaters hold (state, buffers, feed workspace, pending output) */
int flate_hip_debug_device_bytes(flate_hip_handle h, uint64_t* bytes);
/* test seam: device bytes the handle holds as workspace of its passes (the buffers it grows on demand and keeps across
 * calls), not counting the buffers that hold a batch itself -- the staged copies of a host call's input, output, lengths
 * and statuses, and the batch's chunk and block tables -- and not the deflaters' (flate_hip_debug_device_bytes).  A
 * chunk-path batch on two compute streams keeps two slices of its largest pass, whatever the number of passes. */
int flate_hip_debug_workspace_bytes(flate_hip_handle h, uint64_t* bytes);
/* test seam: which path finished the streams of the handle's last flate_hip_decompress_batch call.  counts[0]: streams
 * the span path decoded whole; counts[1]: streams it took (cut, decoded, summed) and then left to the kernels that
 * follow -- a chain that did not close, a checksum or size that did not match the footer; counts[2]: streams the
 * workgroup-per-stream kernel finished; counts[3]: streams it was launched for and handed on to the wave-per-stream
 * kernel (too short by its rule, irregular, or a checksum that did not match).  Every stream not counted in [0] or
 * [2] was decoded by the wave-per-stream kernel.  Waits for the handle's stream. */
int flate_hip_debug_inflate_paths(flate_hip_handle h, uint64_t counts[4]);
/* test seam: for the handle's last flate_hip_decompressed_sizes call, counts[0]: streams whose size came from a closed
 * chain of spans; counts[1]: streams counted whole by one wave. */
int flate_hip_debug_size_paths(flate_hip_handle h, uint64_t counts[2]);
/* test seam: for the handle's last flate_hip_decompress_members call, counts[0]: streams whose members were found by the
 * scan for candidates; counts[1]: streams that were walked; counts[2]: candidates that were probed and lie on no chain. */
int flate_hip_debug_member_paths(flate_hip_handle h, uint64_t counts[3]);

/* The containers' checksums on their own (container.zig:168-206: std.hash.Crc32 / Adler32 over the raw
 * input): container 1 = CRC-32, 2 = Adler-32 of a host buffer, computed by the checksum kernels; and the
 * checksum of a concatenation from the checksums of its parts (value_b over len_b bytes follows value_a).
 * The streaming compressor wrappers use them to write the footer of a stream they compressed piece by
 * piece (flate_hip_compress_flush on the tail of the stream only). */
int flate_hip_checksum(flate_hip_handle h, const uint8_t* data, uint64_t n, int container, uint32_t* value);
uint32_t flate_hip_checksum_combine(int container, uint32_t value_a, uint32_t value_b, uint64_t len_b);

const char* flate_hip_status_name(int status);
const char* flate_hip_last_error(flate_hip_handle h);
const char* flate_hip_version(void);

/* ---- measurement hooks (bench.py / tests) ---- */
/* When enabled every kernel launch is bracketed by hipEvents on the launch stream.
 * flate_hip_profile_read synchronises, folds the pending events into per-kernel
 * totals and returns them: names[i], total_ms[i], launches[i] for i < return value
 * (at most cap).  flate_hip_profile_reset clears the totals. */
int flate_hip_profile_enable(flate_hip_handle h, int enable);
int flate_hip_profile_read(flate_hip_handle h, const char** names, double* total_ms,
                           uint64_t* launches, int cap);
int flate_hip_profile_reset(flate_hip_handle h);

/* ---- test seam (the reference's own seam is the BlockWriterType parameter of
 * Deflate, deflate.zig:118-121: "so we can change that in test to test just
 * tokenization part").  After a level 4..9 compress_batch call, copies the token
 * list the tokenizer kernels produced for chunk `chunk` (same 32-bit token
 * encoding as the oracle: bit23 kind, bits15-22 len-3 / literal, bits0-14
 * dist-1) into host memory.  Returns the token count or a negative error. */
int64_t flate_hip_debug_tokens(flate_hip_handle h, uint32_t chunk, uint32_t* tokens, uint64_t cap);

/* ---- test seam for the block writer alone (the reference tests it the same way: token lists
 * straight into BlockWriter.write / dynamicBlock, block_writer.zig:599-706).  Runs the DEVICE
 * planner, offset scan and bit packer on a caller-supplied token list (<= 32768 tokens, encoding as
 * above) and optional raw input (`input` NULL = the Zig `null`: the block cannot be stored) and
 * writes the block, padded to a byte as BlockWriter.flush does, to host memory.  dynamic_only = 1
 * plans the block as BlockWriter.dynamicBlock does (block_writer.zig:395-432). */
int flate_hip_debug_write_block(flate_hip_handle h, const uint32_t* tokens, uint32_t n_tokens,
                                const uint8_t* input, uint32_t input_len, int eof, int dynamic_only,
                                uint8_t* out, uint64_t out_cap, uint64_t* out_len);

/* The same seam for n blocks in one call, each a chunk of its own, and with a choice of the bit packer: block i has
 * tokens[tok_off[i] .. tok_off[i + 1]), the raw input input[in_off[i] .. in_off[i + 1]) when has_input[i] (else the
 * Zig `null`), the final-block bit eof[i], and is written to out[slot_off[i] .. + slot_cap[i]); out_len[i] is its
 * byte count.  tok_off and in_off have n + 1 entries.  `out` and out_cap are multiples of 4; slot starts may have
 * any residue mod 4, slots must not overlap and are expected to leave 8 spare bytes behind a block (neighbours then
 * share no dword).  Bytes of a slot behind out_len[i] are unspecified.
 * encoder 0: k_encode<true>, a workgroup per block (few blocks, long streams); encoder 1: k_encode_wave, a wave per
 * block (what a batch of 8192 or more plan slots runs).  paired = 1 lays the plan slots out as the chunk path does:
 * two a chunk, the second one unused, visited by k_plan and k_encode_wave in their first-slots-first order; paired = 0:
 * one slot a chunk, plain order.  Fails with FLATE_HIP_E_INVALID_ARG when a block does not fit its slot. */
int flate_hip_debug_write_blocks(flate_hip_handle h, uint32_t n, const uint32_t* tokens, const uint64_t* tok_off,
                                 const uint8_t* input, const uint64_t* in_off, const uint8_t* has_input,
                                 const uint8_t* eof, int dynamic_only, int encoder, int paired, uint8_t* out,
                                 uint64_t out_cap, const uint64_t* slot_off, const uint64_t* slot_cap,
                                 uint64_t* out_len);

/* Tuning aid: shader-clock timestamps that workgroup 0 of the tokenizer kernels took at its
 * phase boundaries during the last call (slots: sort 0-7, match 8-10, parse 16-23). */
int flate_hip_debug_phase_cycles(flate_hip_handle h, uint64_t* out, int n);

/* The FLATE_HIP_* tuning variables are read once, in flate_hip_create: no call path reads the
 * environment.  This reads them again (the test suite changes them between calls of one handle). */
int flate_hip_debug_reload_env(flate_hip_handle h);

#ifdef __cplusplus
}
#endif
#endif
