// kernels_index.h -- the seek index (flate_hip_index_build, flate_hip_decompress_ranges; host side: index_plan.h).
//
// k_index_walk     the size probe's member loop (fl_sz_member) with a point emitter at its block-start line: one wave per
//                  walk job, which is a whole stream or a stretch of one that starts at a block start with a known output
//                  base.  Nothing is decoded into memory.
// k_index_windows  the points' windows, copied out of the bytes the build has just decoded.
// k_inflate_range  the wave-per-stream decoder of kernels_inflate.h (its output with a dictionary in front, fl_inf_out_dict),
//                  started at a point's bit with the point's window as the dictionary and stopped once skip + len bytes
//                  are there; it decodes into a scratch slot.
// k_range_pack     the range's bytes from the scratch slot to the caller's slot (fl_gather_one: 16-byte stores).
#pragma once
#include "index_plan.h"
#include "kernels_block.h"
#include "kernels_inflate.h"
#include "kernels_inflate_size.h"

// one walk: the blocks of `stream` from start_bit up to the first block start at or behind stop_bit
struct fl_idx_walk_job {
    uint64_t start_bit;  // a block starts here (0 with first: the container's header does)
    uint64_t stop_bit;   // ~0: to the end of the member
    uint64_t base;       // output bytes in front of the first block
    uint64_t point0;     // where this walk's points go in the call's arrays
    uint64_t cap;        // ... and how many of them there is room for
    uint32_t stream;
    uint32_t first;
};
struct fl_idx_walk_rec {
    uint64_t n_points;  // found (more than cap: the rest was not written)
    uint64_t out_len;   // bytes the walk's blocks produce
    int32_t status;
    uint32_t final_seen;
};

// The point rule at the block-start line (index_plan.h, fl_idx_point_rule): a block start is a point when the block in
// front of it holds a grid line; the stream's first block is point 0.  Whether the first block of a walk that starts
// inside the stream is a point is the business of the walk in front of it, which is told its own stop.
struct fl_idx_emit {
    enum { ON = 1 };
    uint64_t spacing, base, prev, cap, n;
    uint64_t* in_bit;
    uint64_t* out_pos;
    uint32_t lane;
    bool have_prev, first;
    __device__ __forceinline__ void block_start(uint64_t bit, uint64_t counted) {
        const uint64_t pos = base + counted;
        const bool is = have_prev ? pos / spacing > prev / spacing : first;
        prev = pos;
        have_prev = true;
        if (is) {
            if (n < cap && lane == 0) {
                in_bit[n] = bit;
                out_pos[n] = pos;
            }
            n++;
        }
    }
    __device__ __forceinline__ void stored_block(uint64_t, uint32_t) {}
};

// One wave per walk job.  The loop is the span instance of the size probe's (a whole stream is the span from its first
// byte that never stops): a match that reaches in front of the walk's own bytes is not refused -- the build has decoded
// the stream and only streams it found good are walked.
__global__ __launch_bounds__(64, FL_SZ_WAVES) void k_index_walk(const uint8_t* __restrict__ in, const fl_chunk* __restrict__ chunks,
                                                                 int container, int flags, uint64_t spacing,
                                                                 const fl_idx_walk_job* __restrict__ jobs, fl_idx_walk_rec* __restrict__ recs,
                                                                 uint64_t* __restrict__ pt_bit, uint64_t* __restrict__ pt_pos) {
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
    fl_idx_emit em;
    em.spacing = spacing;
    em.base = jb.base;
    em.prev = 0;
    em.cap = jb.cap;
    em.n = 0;
    em.in_bit = pt_bit + jb.point0;
    em.out_pos = pt_pos + jb.point0;
    em.lane = lane;
    em.have_prev = false;
    em.first = first;
    uint32_t final_seen = 0;
    uint64_t end_bit = 0;
    const int rc = fl_sz_member<true, fl_idx_emit>(r, ws, container, flags, lane, first, jb.stop_bit, total_bits, cnt, final_seen, end_bit, &em);
    if (lane == 0) {
        fl_idx_walk_rec rec;
        rec.n_points = em.n;
        rec.out_len = cnt.n;
        rec.status = rc;
        rec.final_seen = final_seen;
        recs[blockIdx.x] = rec;
    }
}

// Window w: len[w] bytes from src_off[w] of the decoded output to dst_off[w] of the index's windows.
__global__ __launch_bounds__(256) void k_index_windows(const uint8_t* __restrict__ out, const uint64_t* __restrict__ src_off,
                                                       const uint64_t* __restrict__ len, uint8_t* __restrict__ win,
                                                       const uint64_t* __restrict__ dst_off) {
    fl_gather_one(out, src_off, len, win, dst_off, blockIdx.x, blockIdx.y, gridDim.y);
}

// one range of a flate_hip_decompress_ranges pass
struct fl_range_job {
    uint64_t in_off;    // the stream's first byte
    uint64_t in_bit;    // the point's
    uint64_t win_off;   // the point's window among the index's windows
    uint64_t slot_off;  // the scratch slot (FL_IDX_SLOT_ALIGN; need + FL_IDX_SLACK bytes at least)
    uint64_t need;      // bytes to decode from the point: skip + len
    uint64_t len;       // bytes the range delivers
    uint32_t in_len;
    uint32_t win_len;
    int32_t status;     // decode == 0: the range's status (it delivers nothing)
    uint32_t decode;
};

// One wave per range.  The slot has FL_IDX_SLACK bytes behind `need`, so the token that covers the range's last byte is
// never refused for room: the decoder stops between two blocks once `need` bytes are there, or inside a block at the
// first token that would cross the slot's end (status 100 from fl_inf_match / fl_inf_literal, with nothing of that token
// written) -- by then more than `need` bytes are there.  A stored block that runs past the end is copied as far as
// `need`.  There is no checksum to compare: what tells that `in` is no longer what the index was built from is a decode
// error, or nothing.
template <uint32_t RING>
__global__ FL_INF_ATTR __launch_bounds__(64, (RING <= 4096u ? FL_INF_WAVES : 1)) void k_inflate_range(
    const uint8_t* __restrict__ in, const fl_range_job* __restrict__ jobs, int flags, const uint8_t* __restrict__ win,
    uint8_t* __restrict__ scratch, uint64_t* __restrict__ out_len, int32_t* __restrict__ status) {
    __shared__ fl_inflate_ws16 ws_mem;
    __shared__ alignas(8) uint8_t ring_mem[RING];
    __shared__ uint32_t inring_mem[FL_INF_INRING / 4];
    FL_LDS fl_inflate_ws16* ws = (FL_LDS fl_inflate_ws16*)&ws_mem;
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    const fl_range_job jb = jobs[j];
    if (!jb.decode) {
        if (lane == 0) {
            out_len[j] = 0;
            status[j] = jb.status;
        }
        return;
    }
    fl_bitr r;
    r.data = in + jb.in_off;
    r.nbytes = jb.in_len;
    r.lane = lane;
    r.inring = (FL_LDS uint32_t*)inring_mem;
    r.left = (int64_t)((uint64_t)jb.in_len * 8 - jb.in_bit);
    fl_br_seek(r, (uint32_t)(jb.in_bit >> 3));
    fl_br_resync(r);
    fl_inf_out_dict o;
    o.out = scratch + jb.slot_off;
    o.ring = (FL_LDS uint8_t*)ring_mem;
    o.rmask = RING - 1;
    o.near_max = RING - 260;
    o.cap = jb.need + FL_IDX_SLACK;
    o.wp = 0;
    o.flushed = 0;
    o.fenced = 0;
    o.bias = (uint32_t)((uintptr_t)o.out & 7);
    o.dict_end = win + jb.win_off + jb.win_len;
    o.hist_len = jb.win_len;
    fl_inf_seed_ring(o, lane);
    const uint64_t need = jb.need;
    int rc = 0;
    while (fl_uni64(o.wp) < need) {
        uint32_t bfinal, btype;
        if ((rc = (int)fl_uni((uint32_t)fl_br_read(r, 1, bfinal)))) break;
        if ((rc = (int)fl_uni((uint32_t)fl_br_read(r, 2, btype)))) break;
        bfinal = fl_uni(bfinal);
        btype = fl_uni(btype);
        if (btype == 2) {
            if ((rc = (int)fl_uni((uint32_t)fl_inf_dynamic_header(r, ws, flags, lane)))) break;
            for (uint32_t i = lane; i < 80; i += 64) ((FL_LDS uint32_t*)ws->lens)[i] = 0;  // the fast rounds' owner array
            fl_lds_order();
            rc = (int)fl_uni((uint32_t)fl_inf_dynamic(r, ws, o, lane));
        } else if (btype == 0) {
            uint32_t len;
            if ((rc = (int)fl_uni((uint32_t)fl_inf_stored_header(r, len)))) break;
            const uint64_t left = need - fl_uni64(o.wp);
            fl_inf_stored_copy(r, o, (uint64_t)len > left ? (uint32_t)left : len, lane);
        } else if (btype == 1) {
            rc = (int)fl_uni((uint32_t)fl_inf_fixed(r, o, lane));
        } else {
            rc = 12;  // InvalidBlockType
        }
        if (rc || bfinal) break;
    }
    fl_inf_flush(o, o.wp, lane);
    if (lane == 0) {
        const bool got = fl_uni64(o.wp) >= need;
        // (the member ended in front of the range's last byte: these are not the bytes the index was built from)
        const int st = got && (rc == 0 || rc == 100) ? 0 : (rc ? rc : 1);
        out_len[j] = st ? 0 : jb.len;
        status[j] = st;
    }
}

// Range j of the pass: out_len[j] bytes (what k_inflate_range said it delivers) from src_off[j] of the scratch to
// dst_off[j] of the caller's buffer.  Every byte written lies in the first out_len[j] bytes of the range's slot.
__global__ __launch_bounds__(256) void k_range_pack(const uint8_t* __restrict__ scratch, const uint64_t* __restrict__ src_off,
                                                    const uint64_t* __restrict__ out_len, uint8_t* __restrict__ out,
                                                    const uint64_t* __restrict__ dst_off) {
    fl_gather_one(scratch, src_off, out_len, out, dst_off, blockIdx.x, blockIdx.y, gridDim.y);
}
