// CPU shim over flate_amd/csrc/join_plan.h for tests/test_join_plan_cpu.py: the host decisions of
// flate_hip_compress_joined as plain C functions.
#include "../../flate_amd/csrc/join_plan.h"

extern "C" {

uint64_t shim_join_const(int i) {
    switch (i) {
        case 0: return FL_JOIN_MAX_PIECE;
        case 1: return FL_JOIN_MARKER_MAX;
        case 2: return FL_JOIN_SLOT_ALIGN;
        case 3: return FL_JOIN_SLOT_SPARE;
        case 4: return FL_JOIN_MAX_PIECES;
        case 5: return sizeof(fl_join_stream);
        default: return 0;
    }
}

int shim_join_args_ok(uint32_t piece_bytes, int container, int mode) { return fl_join_args_ok(piece_bytes, container, mode) ? 1 : 0; }
uint32_t shim_join_piece_bytes(uint32_t piece_bytes) { return fl_join_piece_bytes(piece_bytes); }
uint32_t shim_join_marker_bytes(uint32_t residue) { return fl_join_marker_bytes(residue); }
uint64_t shim_join_raw_bound(uint64_t n) { return fl_raw_bound(n); }
uint64_t shim_join_bound(uint64_t n, uint32_t piece, int container) { return fl_join_bound(n, piece, container); }
uint64_t shim_join_slot_bytes(uint32_t len) { return fl_join_slot_bytes(len); }
uint64_t shim_join_piece_count(uint64_t n, uint32_t piece) { return fl_join_piece_count(n, piece); }

// the streams of a call: per stream in_off / n / out_off / out_cap / piece0 / n_pieces (6 values); returns the pieces
uint64_t shim_join_layout(const uint64_t* hin, const uint64_t* hout, uint32_t n, uint32_t piece, uint64_t in_shift, uint64_t out_shift,
                          uint64_t* rows) {
    std::vector<fl_join_stream> s;
    const uint64_t total = fl_join_layout(hin, hout, n, piece, in_shift, out_shift, s);
    for (uint32_t i = 0; i < n; i++) {
        uint64_t* r = rows + 6 * i;
        r[0] = s[i].in_off;
        r[1] = s[i].n;
        r[2] = s[i].out_off;
        r[3] = s[i].out_cap;
        r[4] = s[i].piece0;
        r[5] = s[i].n_pieces;
    }
    return total;
}

// piece k of a stream of n bytes that starts at in_off: in_off / in_len / last (no table: a stream may have 2^32 pieces)
void shim_join_piece_of(uint64_t in_off, uint64_t n, uint32_t piece, uint64_t k, uint64_t* out) {
    fl_join_stream s{};
    s.in_off = in_off;
    s.n = n;
    s.n_pieces = fl_join_piece_count(n, piece);
    const fl_join_piece p = fl_join_piece_of(s, k, piece);
    out[0] = p.in_off;
    out[1] = p.in_len;
    out[2] = p.last;
}

// the piece tables of a call of `total` pieces (what shim_join_layout returned): piece -> stream, the total + 1 input
// offsets and scratch slots; returns the scratch bytes
uint64_t shim_join_tables(const uint64_t* hin, const uint64_t* hout, uint32_t n, uint32_t piece, uint64_t total, uint32_t* piece_stream,
                          uint64_t* piece_in, uint64_t* piece_slot) {
    std::vector<fl_join_stream> s;
    if (fl_join_layout(hin, hout, n, piece, 0, 0, s) != total) return ~0ull;
    std::vector<uint32_t> ps;
    std::vector<uint64_t> pin, pslot;
    const uint64_t bytes = fl_join_tables(s, piece, total, ps, pin, pslot);
    if (ps.size() != total || pin.size() != total + 1 || pslot.size() != total + 1) return ~0ull;
    for (uint64_t j = 0; j < total; j++) piece_stream[j] = ps[j];
    for (uint64_t j = 0; j <= total; j++) {
        piece_in[j] = pin[j];
        piece_slot[j] = pslot[j];
    }
    return bytes;
}
}
