// CPU build of the pass schedule of compress_impl (flate_amd/csrc/pass_plan.h).
// TEST INFRASTRUCTURE ONLY: lets the passes a chunk-path batch is cut into, and the workspace bytes per chunk and per
// block they are sized by, be checked without a GPU.  Not linked into libflate_hip.so.
#include "../../flate_amd/csrc/pass_plan.h"

extern "C" {

// the passes of a batch: writes up to `cap` (c0, nc, stream) triples, returns the count; *largest = the largest pass
int shim_pass_schedule(uint64_t n_chunks, uint64_t host_pass_chunks, uint64_t max_pass_chunks, int pinned, int ramp,
                       int planned, uint64_t* out, int cap, uint64_t* largest) {
    fl_pass_cfg c;
    c.n_chunks = n_chunks;
    c.host_pass_chunks = host_pass_chunks;
    c.max_pass_chunks = max_pass_chunks;
    c.pinned = pinned != 0;
    c.ramp = ramp != 0;
    c.planned = planned != 0;
    std::vector<fl_pass> v;
    *largest = fl_pass_schedule(c, v);
    for (int i = 0; i < (int)v.size() && i < cap; i++) {
        out[3 * i] = v[i].c0;
        out[3 * i + 1] = v[i].nc;
        out[3 * i + 2] = v[i].stream;
    }
    return (int)v.size();
}

uint64_t shim_lz_chunk_bytes(int bulk_links) { return fl_lz_chunk_bytes(bulk_links != 0); }
uint64_t shim_block_bytes() { return fl_block_bytes(); }

}  // extern "C"
