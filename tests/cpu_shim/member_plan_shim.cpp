// CPU build of the member finder's rules (flate_amd/csrc/member_plan.h).
// TEST INFRASTRUCTURE ONLY: lets the successor rule, the walk of a stream's chain tile by tile and the table it leaves be
// checked without a GPU.  Not linked into libflate_hip.so.
#include "../../flate_amd/csrc/member_plan.h"

#include <vector>

extern "C" {

int shim_member_scan_tile() { return (int)FL_MEM_SCAN_TILE; }
int shim_member_lds_tile() { return (int)FL_MEM_LDS_TILE; }
int shim_member_least_bytes(int container) { return (int)fl_member_least_bytes(container); }
int shim_member_miss_status(uint64_t bytes_left) { return (int)fl_member_miss_status(bytes_left); }
uint32_t shim_member_stream_of(const uint64_t* off, uint32_t n, uint64_t p) { return fl_member_stream_of(off, n, p); }

// What k_member_chain does for one stream [stream_start, stream_end) whose candidates are pos[0..n) with the probe's
// (status, consumed, size) each: successors, chain, table.  Writes the table (at most n + 1 entries), the stream's status
// as the table implies it (0: the chain is complete; a refused candidate's status; the header rule where the walk left
// the candidates) and the candidates on the chain; returns the table's length.
int shim_member_chain(const uint64_t* pos, const int32_t* status, const uint64_t* consumed, const uint64_t* size, uint32_t n,
                      uint64_t stream_start, uint64_t stream_end, uint32_t* tab_start, uint64_t* tab_size, int32_t* st_out,
                      uint32_t* on_chain) {
    std::vector<uint32_t> succ(n ? n : 1), chain(n ? n : 1), tile(FL_MEM_LDS_TILE);
    for (uint32_t i = 0; i < n; i++) succ[i] = fl_member_successor(pos, n, i, status[i], consumed[i], stream_end);
    const uint32_t first = n && pos[0] == stream_start ? 0u : FL_MEM_MISS;
    uint32_t stop = 0;
    const uint32_t count = fl_member_follow(
        succ.data(), n, first, tile.data(), 0u, 1u, [] {}, [](uint32_t v) { return v; }, chain.data(), &stop);
    const uint32_t m = fl_member_table(chain.data(), count, stop, pos, consumed, size, stream_start, 0u, 1u, tab_start, tab_size);
    *on_chain = count;
    if (stop == FL_MEM_END)
        *st_out = 0;
    else if (stop == FL_MEM_ERR)
        *st_out = status[chain[count - 1]];
    else
        *st_out = fl_member_miss_status(stream_end - (stream_start + tab_start[m - 1]));
    return (int)m;
}

// the members' slots of one stream: m starts
void shim_member_slots(const uint64_t* size, uint32_t m, uint64_t slot_start, uint64_t slot_end, uint64_t* out) {
    fl_member_slots(size, m, slot_start, slot_end, out);
}

// ---- the host's side of flate_hip_decompress_members

// the scan's tiles over [lo, hi) of a buffer at address base; returns 0 where there are too many
int shim_member_scan_tiles(uint64_t base, uint64_t lo, uint64_t hi, int64_t* rel0, uint64_t* n_tiles) {
    fl_member_tiles t;
    const bool ok = fl_member_scan_tiles(base, lo, hi, t);
    *rel0 = t.rel0;
    *n_tiles = t.n_tiles;
    return ok ? 1 : 0;
}

uint64_t shim_member_scan_cap(uint64_t n_cand, uint32_t n_streams) { return fl_member_scan_cap(n_cand, n_streams); }

// toff[0..n]; returns the capacity
uint64_t shim_member_walk_offsets(const uint64_t* hin, uint32_t n, int container, uint64_t* toff) {
    return fl_member_walk_offsets(hin, n, container, toff);
}

int shim_member_count_ok(uint64_t M, uint32_t n_streams, uint64_t cap) { return fl_member_count_ok(M, n_streams, cap) ? 1 : 0; }

// min_ / mout[0..doff[n]]; returns the fault (0: none) and the stream it names
int shim_member_partition(const uint64_t* doff, const uint32_t* mstart, const uint64_t* msize, const uint64_t* vin, const uint64_t* vout,
                          uint32_t n, uint64_t* min_, uint64_t* mout, uint32_t* stream) {
    const fl_member_verdict v = fl_member_partition(doff, mstart, msize, vin, vout, n, min_, mout);
    *stream = v.stream;
    return v.fault;
}

}  // extern "C"
