// CPU build of the inflate entry points' host decisions (flate_amd/csrc/inflate_plan.h).
// TEST INFRASTRUCTURE ONLY: lets the chunk table, the ring rule, the pinned sub-batches, the k_inflate_par rule, the span
// pool's bound, the copy-out plan and the rules of the resumable inflater's host feeds be checked without a GPU.  Not linked
// into libflate_hip.so.
#include "../../flate_amd/csrc/inflate_plan.h"

#include <cstring>

extern "C" {

// 0: small ring, 1: large ring, 2: the longest input of a stream
uint64_t shim_inflate_const(int i) {
    const uint64_t v[] = {FL_INF_RING_SMALL, FL_INF_RING_LARGE, FL_INF_MAX_IN_BYTES};
    return v[i];
}

int shim_inflate_ring_large(int64_t knob, uint32_t n_streams) { return fl_inflate_ring_large(knob, n_streams) ? 1 : 0; }

int shim_inflate_pin_io(int in_pinned, int out_pinned, uint64_t in_bytes, uint64_t out_bytes, uint32_t n_streams, uint64_t host_pass_chunks) {
    return fl_inflate_pin_io(in_pinned != 0, out_pinned != 0, in_bytes, out_bytes, n_streams, (size_t)host_pass_chunks) ? 1 : 0;
}

uint32_t shim_inflate_sub_batch(uint32_t n_streams, uint64_t host_pass_chunks) {
    return fl_inflate_sub_batch(n_streams, (size_t)host_pass_chunks);
}

// out: min_bytes, n_big, taken; returns use
int shim_inflate_par(const uint32_t* in_len, const uint64_t* out_cap, const uint32_t* skip, uint32_t n, int64_t knob, int flags,
                     uint64_t* out) {
    std::vector<fl_chunk> chunks(n, fl_chunk{});
    for (uint32_t i = 0; i < n; i++) {
        chunks[i].in_len = in_len[i];
        chunks[i].out_cap = out_cap[i];
        chunks[i].skip = skip[i];
    }
    const fl_inflate_par p = fl_inflate_par_plan(chunks.data(), n, knob, flags);
    out[0] = p.min_bytes;
    out[1] = p.n_big;
    out[2] = p.taken;
    return p.use ? 1 : 0;
}

uint32_t shim_inflate_oversize(const uint64_t* hin, uint32_t n) { return fl_inflate_oversize(hin, n); }

// rows: n x 5 -- in_off, out_off, out_cap, in_len, and 1 where every other byte of the entry is 0; hout may be null
int shim_inflate_chunks(const uint64_t* hin, const uint64_t* hout, uint32_t n, uint64_t in_shift, uint64_t out_shift, uint64_t* rows) {
    std::vector<fl_chunk> chunks;
    if (!fl_inflate_chunks(hin, hout, n, in_shift, out_shift, chunks)) return 0;
    if (chunks.size() != n) return -1;
    for (uint32_t i = 0; i < n; i++) {
        fl_chunk c = chunks[i];
        rows[5 * i + 0] = c.in_off;
        rows[5 * i + 1] = c.out_off;
        rows[5 * i + 2] = c.out_cap;
        rows[5 * i + 3] = c.in_len;
        c.in_off = c.out_off = c.out_cap = 0;
        c.in_len = 0;
        const fl_chunk zero{};
        rows[5 * i + 4] = memcmp(&c, &zero, sizeof c) == 0;
    }
    return 1;
}

int shim_inflate_pool_release(uint64_t pool_bytes) { return fl_inflate_pool_release(pool_bytes) ? 1 : 0; }

// out: total, end; returns the kind (0 nothing, 1 dense, 2 packed)
int shim_copy_out_plan(const uint64_t* hout, const uint64_t* out_len, uint32_t n, uint64_t* out) {
    const fl_copy_out p = fl_copy_out_plan(hout, out_len, n);
    out[0] = p.total;
    out[1] = p.end;
    return p.kind;
}

// ---- the resumable inflater's host feeds
int shim_inflater_slots_ok(const uint64_t* in_off, const uint64_t* out_off, const uint8_t* final_, uint32_t n) {
    return fl_inflater_slots_ok(in_off, out_off, final_, n) ? 1 : 0;
}

// hin, hout: n + 1 entries each; returns 0 where the tables do not come back with that length
int shim_inflater_rebase(const uint64_t* in_off, const uint64_t* out_off, uint32_t n, uint64_t* hin, uint64_t* hout) {
    std::vector<uint64_t> a(3, 77), b;  // (what they held must go)
    fl_inflater_rebase(in_off, out_off, n, a, b);
    if (a.size() != (size_t)n + 1 || b.size() != (size_t)n + 1) return 0;
    memcpy(hin, a.data(), 8 * a.size());
    memcpy(hout, b.data(), 8 * b.size());
    return 1;
}

int shim_inflater_copy_each(uint32_t n) { return fl_inflater_copy_each(n) ? 1 : 0; }

}  // extern "C"
