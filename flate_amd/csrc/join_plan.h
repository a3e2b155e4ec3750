// join_plan.h -- the host decisions of flate_hip_compress_joined (flate_hip.hip, which only carries them out): the
// checks of the call's arguments (fl_join_args_ok), how a stream is cut into pieces (fl_join_piece_count,
// fl_join_piece_of), the streams and pieces of a call (fl_join_layout, fl_join_tables), the bound
// (fl_join_bound), where every piece's scratch slot lies (fl_join_slot_bytes) and how long a sync-flush marker is behind
// a block that ends at a given bit (fl_join_marker_bytes, shared with k_join_open).
//
// A joined stream is  header, F(piece_0) .. F(piece_{P-2}), L(piece_{P-1}), footer:  every piece is compressed with no
// history, as a raw stream of its own by the chunk path; every piece but the last has its final-block bit cleared and a
// sync-flush marker appended (what a fresh reference compressor has written after write(piece); flush()), so the pieces
// end on byte boundaries and simply follow each other.  Pieces of one stream lie back to back in the input, and so do the
// streams of a call: the pieces of a call are a batch of the shape flate_hip_compress_batch takes.
// Plain C++ (no HIP): tests/cpu_shim compiles it for the CPU tests and tests/host_cpp/test_join_plan.cpp walks it under
// sanitizers.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/flate_hip.h"
#include "flate_common.h"

#define FL_JOIN_MAX_PIECE 65535u  // a piece takes the chunk path: the reference's window never slides over it
#define FL_JOIN_MARKER_MAX 5u
// a piece's scratch slot: a multiple of 16 bytes with at least 16 spare ones behind the piece and its marker (the bit
// packer and the copy kernel touch whole dwords: neighbours share none)
#define FL_JOIN_SLOT_ALIGN 16u
#define FL_JOIN_SLOT_SPARE 16u

// Bytes of the sync-flush marker (block_writer.zig:276-278: an empty stored block) behind a block that ends `residue`
// bits into a byte: its three header bits fit the block's last byte when 1..5 padding bits are left there and the marker
// is 00 00 ff ff; at residue 0 (a stored block ends so), 6 or 7 the header takes a byte of its own: 00 00 00 ff ff.
FL_HD uint32_t fl_join_marker_bytes(uint32_t residue) {
    residue &= 7u;
    return (residue == 0u || residue >= 6u) ? 5u : 4u;
}

inline uint32_t fl_join_piece_bytes(uint32_t piece_bytes) { return piece_bytes ? piece_bytes : FL_JOIN_MAX_PIECE; }

// What the call may be given: levels 4..9, a container, a piece of at most 65535 bytes (0: 65535).  False:
// FLATE_HIP_E_INVALID_ARG.
inline bool fl_join_args_ok(uint32_t piece_bytes, int container, int mode) {
    if (mode < 4 || mode > 9) return false;
    if (container < FLATE_HIP_RAW || container > FLATE_HIP_ZLIB) return false;
    return piece_bytes <= FL_JOIN_MAX_PIECE;
}

inline uint32_t fl_join_hdr_bytes(int container) { return container == FLATE_HIP_GZIP ? 10u : container == FLATE_HIP_ZLIB ? 2u : 0u; }
inline uint32_t fl_join_ftr_bytes(int container) { return container == FLATE_HIP_GZIP ? 8u : container == FLATE_HIP_ZLIB ? 4u : 0u; }

// flate_hip_compress_bound(n, FLATE_HIP_RAW, any mode): stored blocks cost 5 bytes per 65535 (and a possibly empty trailing
// one), a Huffman block never beats that bound by more than its header; slack for the Q1 seam
inline uint64_t fl_raw_bound(uint64_t n) { return n + (n / 32768 + 2) * 16 + 64 + n / 64; }

// pieces of a stream of n bytes: an empty stream is one empty piece
inline uint64_t fl_join_piece_count(uint64_t n, uint32_t piece) { return n == 0 ? 1 : n / piece + (n % piece != 0); }

// flate_hip_joined_bound: header, every piece's raw bound and the longest marker, footer.  Closed form: P - 1 whole pieces
// and the last one (a stream of 2^32 + 5 bytes in pieces of one byte has 2^32 + 5 of them).
inline uint64_t fl_join_bound(uint64_t n, uint32_t piece, int container) {
    const uint64_t P = fl_join_piece_count(n, piece);
    const uint64_t last = n - (P - 1) * piece;
    return fl_join_hdr_bytes(container) + (P - 1) * (fl_raw_bound(piece) + FL_JOIN_MARKER_MAX) + (fl_raw_bound(last) + FL_JOIN_MARKER_MAX) +
           fl_join_ftr_bytes(container);
}

// the scratch slot of a piece of `len` bytes
inline uint64_t fl_join_slot_bytes(uint32_t len) {
    const uint64_t need = fl_raw_bound(len) + FL_JOIN_MARKER_MAX + FL_JOIN_SLOT_SPARE;
    return (need + FL_JOIN_SLOT_ALIGN - 1) & ~(uint64_t)(FL_JOIN_SLOT_ALIGN - 1);
}

// One stream of the call (host and device)
struct fl_join_stream {
    uint64_t in_off;    // its first byte in `in`
    uint64_t n;         // its bytes (any number: a joined stream has no 32-bit positions)
    uint64_t out_off;   // its slot in `out` ...
    uint64_t out_cap;   // ... and the slot's size
    uint64_t piece0;    // its first piece among the call's pieces
    uint64_t n_pieces;  // fl_join_piece_count(n, piece)
};

// piece k of a stream
struct fl_join_piece {
    uint64_t in_off;  // its first byte in `in`
    uint32_t in_len;
    uint32_t last;    // the stream's last piece: it keeps its final-block bit and gets no marker
};
inline fl_join_piece fl_join_piece_of(const fl_join_stream& s, uint64_t k, uint32_t piece) {
    fl_join_piece p;
    const uint64_t a = k * piece, b = a + piece < s.n ? a + piece : s.n;
    p.in_off = s.in_off + a;
    p.in_len = (uint32_t)(b - a);
    p.last = k + 1 == s.n_pieces ? 1u : 0u;
    return p;
}

// The streams of a call from its n_streams + 1 ascending input and output offsets, with the staging shifts taken off.
// Returns the call's number of pieces (a call may have at most FL_JOIN_MAX_PIECES: the pieces are one batch of the chunk
// path, and a grid has a workgroup per piece).
inline uint64_t fl_join_layout(const uint64_t* hin, const uint64_t* hout, uint32_t n_streams, uint32_t piece, uint64_t in_shift,
                               uint64_t out_shift, std::vector<fl_join_stream>& streams) {
    streams.assign(n_streams, fl_join_stream{});
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_streams; i++) {
        fl_join_stream& s = streams[i];
        s.in_off = hin[i] - in_shift;
        s.n = hin[i + 1] - hin[i];
        s.out_off = hout[i] - out_shift;
        s.out_cap = hout[i + 1] - hout[i];
        s.piece0 = total;
        s.n_pieces = fl_join_piece_count(s.n, piece);
        total += s.n_pieces;
    }
    return total;
}
#define FL_JOIN_MAX_PIECES 0x7fffffffull

// The piece tables of a call (total <= FL_JOIN_MAX_PIECES pieces): piece -> stream, the total + 1 ascending input offsets
// of the pieces (a batch of the chunk path) and the total + 1 offsets of their scratch slots.  Returns the scratch bytes.
inline uint64_t fl_join_tables(const std::vector<fl_join_stream>& streams, uint32_t piece, uint64_t total, std::vector<uint32_t>& piece_stream,
                               std::vector<uint64_t>& piece_in, std::vector<uint64_t>& piece_slot) {
    piece_stream.resize(total);
    piece_in.resize(total + 1);
    piece_slot.resize(total + 1);
    uint64_t j = 0, slot = 0, in_end = 0;
    for (size_t i = 0; i < streams.size(); i++) {
        const fl_join_stream& s = streams[i];
        for (uint64_t k = 0; k < s.n_pieces; k++, j++) {
            const fl_join_piece p = fl_join_piece_of(s, k, piece);
            piece_stream[j] = (uint32_t)i;
            piece_in[j] = p.in_off;
            piece_slot[j] = slot;
            slot += fl_join_slot_bytes(p.in_len);
        }
        in_end = s.in_off + s.n;
    }
    piece_in[j] = in_end;
    piece_slot[j] = slot;
    return slot;
}
