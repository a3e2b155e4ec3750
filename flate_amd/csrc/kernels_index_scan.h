// kernels_index_scan.h -- flate_hip_index_scan (host side: index_scan_plan.h): the fresh points of streams written
// elsewhere, found without decoding anything into memory.
//
// k_index_scan   the size probe's member loop (fl_sz_member) over the walk jobs of k_index_walk (kernels_index.h), one
//                wave per job, with an emitter that knows a flush marker's trailer when a block start follows it, keeps
//                the marks of its own walk by the cell comparison, and measures how far the matches behind every kept
//                mark reach in front of it.
#pragma once
#include "index_scan_plan.h"
#include "kernels_index.h"

struct fl_ixs_walk_rec {
    uint64_t n_entries;  // listed (more than the job's cap: the rest was not written)
    uint64_t out_len;    // bytes the walk's blocks produce
    uint64_t last_mark;  // has_mark: where the walk's last mark lies, kept or not
    int32_t status;
    uint32_t final_seen;
    uint32_t has_mark;
    uint32_t pad;
};

// The emitter at the block-start line.  Entry 0 is the walk's start.  A block start behind an empty stored block without
// BFINAL is a mark; it is kept when the mark in front of it (block 0 in a stream's first walk) lies in an earlier cell,
// and a walk that starts inside the stream keeps its first mark whatever its cell (index_scan_plan.h: the host has the
// last mark in front of it).  At a kept mark the open entry gets its need and the count starts over: cnt->n is the bytes
// behind the newest kept mark, `acc` those in front of it, and cnt->need what fl_sz_match and the first 32 KiB of
// fl_sz_fast_round measure -- how far a match reaches in front of the count's origin.
struct fl_ixs_emit {
    enum { ON = 1 };
    uint64_t spacing, base, acc, prev, cap, n, last_mark;
    fl_ixs_entry* ent;
    fl_sz_count<true>* cnt;
    uint32_t lane;
    bool have_prev, after_marker, has_mark;
    __device__ __forceinline__ void stored_block(uint64_t len, uint32_t bfinal) { after_marker = len == 0 && !bfinal; }
    __device__ __forceinline__ void block_start(uint64_t bit, uint64_t counted) {
        const uint64_t pos = base + acc + counted;
        const bool mark = after_marker;
        after_marker = false;
        if (n == 0) {  // the walk's start: what lies in front of it is the business of the walk before
            if (cap > 0 && lane == 0) {
                ent[0].in_bit = bit;
                ent[0].out_pos = pos;
            }
            n = 1;
            return;
        }
        if (!mark) return;
        const bool is = have_prev ? pos / spacing > prev / spacing : true;
        prev = pos;
        have_prev = true;
        last_mark = pos;
        has_mark = true;
        if (is) {
            if (lane == 0) {
                if (n - 1 < cap) ent[n - 1].need = cnt->need;
                if (n < cap) {
                    ent[n].in_bit = bit;
                    ent[n].out_pos = pos;
                }
            }
            n++;
            acc += counted;
            cnt->n = 0;
            cnt->need = 0;
        }
    }
};

// One wave per walk job, as k_index_walk: a match that reaches in front of the walk's own bytes is recorded, not
// refused -- the probe has found the stream good.
__global__ __launch_bounds__(64, FL_SZ_WAVES) void k_index_scan(const uint8_t* __restrict__ in, const fl_chunk* __restrict__ chunks,
                                                                 int container, int flags, uint64_t spacing,
                                                                 const fl_idx_walk_job* __restrict__ jobs, fl_ixs_walk_rec* __restrict__ recs,
                                                                 fl_ixs_entry* __restrict__ entries) {
    __shared__ fl_inflate_ws16 ws_mem;
    __shared__ uint32_t inring_mem[FL_INF_INRING / 4];
    FL_LDS fl_inflate_ws16* ws = (FL_LDS fl_inflate_ws16*)&ws_mem;
    const uint32_t lane = threadIdx.x;
    const fl_idx_walk_job jb = jobs[blockIdx.x];
    const fl_chunk ck = chunks[jb.stream];
    const bool first = jb.first != 0;
    fl_bitr r;
    r.data = in + ck.in_off;
    r.nbytes = ck.in_len;
    r.lane = lane;
    r.inring = (FL_LDS uint32_t*)inring_mem;
    const uint64_t total_bits = (uint64_t)ck.in_len * 8;
    r.left = (int64_t)(total_bits - (first ? 0ull : jb.start_bit));
    fl_br_seek(r, first ? 0u : (uint32_t)(jb.start_bit >> 3));
    if (!first) fl_br_resync(r);
    fl_sz_count<true> cnt;
    cnt.n = 0;
    cnt.need = 0;
    fl_ixs_emit em;
    em.spacing = spacing;
    em.base = jb.base;
    em.acc = 0;
    em.prev = 0;
    em.cap = jb.cap;
    em.n = 0;
    em.last_mark = 0;
    em.ent = entries + jb.point0;
    em.cnt = &cnt;
    em.lane = lane;
    em.have_prev = first;  // (block 0 is the rule's pos[0])
    em.after_marker = false;
    em.has_mark = false;
    uint32_t final_seen = 0;
    uint64_t end_bit = 0;
    const int rc = fl_sz_member<true, fl_ixs_emit>(r, ws, container, flags, lane, first, jb.stop_bit, total_bits, cnt, final_seen, end_bit, &em);
    if (lane == 0) {
        if (em.n >= 1 && em.n - 1 < em.cap) em.ent[em.n - 1].need = cnt.need;
        fl_ixs_walk_rec rec;
        rec.n_entries = em.n;
        rec.out_len = em.acc + cnt.n;
        rec.last_mark = em.last_mark;
        rec.status = rc;
        rec.final_seen = final_seen;
        rec.has_mark = em.has_mark ? 1u : 0u;
        rec.pad = 0;
        recs[blockIdx.x] = rec;
    }
}
