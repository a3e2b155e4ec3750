// kernels_index_parts.h -- the fresh seek index (flate_hip_compress_joined_indexed, flate_hip_decompress_ranges on an
// index of that kind; host side: index_parts_plan.h).
//
// k_join_points    the places k_join_scan gave the pieces that are points, collected into one array for the host.
// k_inflate_part   the wave-per-stream decoder of kernels_inflate.h started at a point of a fresh index -- a piece start:
//                  a byte boundary with no history in front -- and stopped once skip + len bytes are there.  It decodes
//                  into a scratch slot, or, a direct part, straight into the caller's slot.
// k_range_settle   every range's status and length from the statuses of its parts.
// (k_range_pack of kernels_index.h copies the scratch parts to the callers' slots.)
#pragma once
#include "index_parts_plan.h"
#include "kernels_index.h"

// place[q] = piece_dst[which[q]]: what the host reads back is 8 bytes a point, not 8 bytes a piece
__global__ __launch_bounds__(256) void k_join_points(const uint64_t* __restrict__ piece_dst, const uint64_t* __restrict__ which, uint64_t n,
                                                     uint64_t* __restrict__ place) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < n) place[q] = piece_dst[which[q]];
}

// one part of a pass of flate_hip_decompress_ranges on a fresh index
struct fl_part_job {
    uint64_t in_off;   // the stream's first byte
    uint64_t in_bit;   // the point's
    uint64_t dst_off;  // direct: the part's place in the caller's buffer; else its scratch slot (FL_IDX_SLOT_ALIGN; need + FL_IDX_SLACK bytes at least)
    uint64_t need;     // bytes to decode from the point: skip + len
    uint64_t len;      // bytes the part delivers
    uint32_t in_len;
    uint32_t direct;
};
// one range of the call, for k_range_settle
struct fl_range_rec {
    uint64_t part0, n_parts;  // n_parts == 0: status is the range's, it delivers nothing
    uint64_t len;             // the clipped length
    int32_t status;
    uint32_t pad;
};

// One wave per part.  The output starts with no history (plain fl_inf_out: a match that reaches in front of the part's
// point is InvalidMatch, nothing in front of it is read).  A scratch part is k_inflate_range's case: the slot has
// FL_IDX_SLACK bytes behind `need`, the decoder stops between two blocks once `need` bytes are there or at the first
// token that would cross the slot's end.  A direct part has a cap of exactly `need` = its length: the piece structure
// ends a block there, and no token that would cross it is written, so fl_inf_flush -- whole 8-byte words inside
// [flushed, upto), the ragged head and tail byte by byte -- and the stored copy (byte by byte) never store outside the
// part, whatever its alignment: the waves of adjacent parts of one slot run at the same time.
// part_len[p]: the bytes the part left in scratch for k_range_pack (0: a direct part, or one that failed).
template <uint32_t RING>
__global__ FL_INF_ATTR __launch_bounds__(64, (RING <= 4096u ? FL_INF_WAVES : 1)) void k_inflate_part(
    const uint8_t* __restrict__ in, const fl_part_job* __restrict__ jobs, int flags, uint8_t* __restrict__ scratch,
    uint8_t* __restrict__ out, uint64_t* __restrict__ part_len, int32_t* __restrict__ part_status) {
    __shared__ fl_inflate_ws16 ws_mem;
    __shared__ alignas(8) uint8_t ring_mem[RING];
    __shared__ uint32_t inring_mem[FL_INF_INRING / 4];
    FL_LDS fl_inflate_ws16* ws = (FL_LDS fl_inflate_ws16*)&ws_mem;
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    const fl_part_job jb = jobs[j];
    fl_bitr r;
    r.data = in + jb.in_off;
    r.nbytes = jb.in_len;
    r.lane = lane;
    r.inring = (FL_LDS uint32_t*)inring_mem;
    r.left = (int64_t)((uint64_t)jb.in_len * 8 - jb.in_bit);
    fl_br_seek(r, (uint32_t)(jb.in_bit >> 3));
    fl_br_resync(r);
    fl_inf_out o;
    o.out = (jb.direct ? out : scratch) + jb.dst_off;
    o.ring = (FL_LDS uint8_t*)ring_mem;
    o.rmask = RING - 1;
    o.near_max = RING - 260;
    o.cap = jb.direct ? jb.need : jb.need + FL_IDX_SLACK;
    o.wp = 0;
    o.flushed = 0;
    o.fenced = 0;
    o.bias = (uint32_t)((uintptr_t)o.out & 7);
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
        // (the stream ended in front of the part's last byte: these are not the bytes the index was made for)
        const int st = got && (rc == 0 || rc == 100) ? 0 : (rc ? rc : 1);
        part_len[j] = st || jb.direct ? 0 : jb.len;
        part_status[j] = st;
    }
}

// One wave per range: the first non-zero status among its parts, which lie in stream order, is the range's; with none
// it delivers its clipped length.
__global__ __launch_bounds__(64) void k_range_settle(const fl_range_rec* __restrict__ ranges, const int32_t* __restrict__ part_status,
                                                     uint64_t* __restrict__ out_len, int32_t* __restrict__ status) {
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    const fl_range_rec rr = ranges[j];
    uint64_t bad = ~0ull;  // the first part of this lane's that failed
    for (uint64_t k = lane; k < rr.n_parts && bad == ~0ull; k += 64)
        if (part_status[rr.part0 + k] != 0) bad = k;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t other = __shfl_xor(bad, d, 64);
        bad = other < bad ? other : bad;
    }
    if (lane == 0) {
        const int32_t st = rr.n_parts == 0 ? rr.status : (bad != ~0ull ? part_status[rr.part0 + bad] : 0);
        status[j] = st;
        out_len[j] = st ? 0 : rr.len;
    }
}
