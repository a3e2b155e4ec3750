// CPU build of the host arithmetic of a resumable huffman-only / store-only feed (flate_amd/csrc/deflater_plan.h).
// TEST INFRASTRUCTURE ONLY: lets the block schedule the deflater builds on the host be checked against the one-shot
// block lists and the oracle.  Not linked into libflate_hip.so.
#include "../../flate_amd/csrc/deflater_plan.h"

extern "C" {

// blocks of one feed: writes up to `cap` (start, len, flags) triples, returns the count; *keep = bytes left buffered
int shim_dfl_blocks(uint32_t bl, uint32_t n, int op, uint32_t* out, int cap, uint32_t* keep) {
    std::vector<fl_sblock> v;
    *keep = fl_dfl_blocks(bl, n, op, v);
    for (int i = 0; i < (int)v.size() && i < cap; i++) {
        out[3 * i] = v[i].start;
        out[3 * i + 1] = v[i].len;
        out[3 * i + 2] = v[i].flags;
    }
    return (int)v.size();
}

int shim_dfl_checksum_units(uint32_t bl, uint32_t n, uint32_t* out, int cap) {
    std::vector<fl_sblock> v;
    fl_dfl_checksum_units(bl, n, v);
    for (int i = 0; i < (int)v.size() && i < cap; i++) {
        out[2 * i] = v[i].start;
        out[2 * i + 1] = v[i].len;
    }
    return (int)v.size();
}

uint64_t shim_dfl_out_bound(uint32_t bl, uint32_t n) { return fl_dfl_out_bound(bl, n); }
}
