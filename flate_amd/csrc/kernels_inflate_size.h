// kernels_inflate_size.h -- the size probe (flate_hip_decompressed_sizes): how many bytes a stream inflates to, without
// inflating it.  One wavefront per stream, or per span of a long stream (size_plan.h).
//
// Bit reader, container header, dynamic block header with its table build, the symbol decoders of both codes and the
// front of a round are those of kernels_inflate.h, called as they are with a counter in the output's place (fl_sink_*).
// A literal adds 1 to a 64-bit counter, a match its length after the checks of fl_inf_match, a stored block its LEN.
// Nothing is produced: no output ring, no flush, no store except the three result words, and the footer is read but not
// compared (there are no bytes to sum).  What a stream keeps in LDS is the decoder tables and the staged input, 5 KiB:
// 32 streams per CU instead of k_inflate's 20.
//
// A dynamic block is counted in rounds of the kind fl_inf_fast_round decodes in: every lane decodes the token that
// would start at "current bit + lane", the chain of real token starts is walked with one scalar read per token, and the
// bytes of the round are the sum of the chain members' lengths -- there is no copy phase.  The only check that needs a
// token's place in the output, distance against the bytes produced so far, matters during the first 32 KiB alone.
// Everything unusual takes the symbol-at-a-time loop, which keeps the reference's order of errors.
#pragma once
#include "kernels_inflate.h"
#include "size_plan.h"

// SPAN: the count starts inside the stream; a distance beyond the span's own bytes is recorded, not refused
template <bool SPAN>
struct fl_sz_count {
    uint64_t n;     // bytes produced so far
    uint64_t need;  // SPAN: largest distance - n over the matches so far
};

// fl_inf_match's checks, and its order: a distance beyond the bytes produced so far is InvalidMatch
template <bool SPAN>
__device__ __forceinline__ int fl_sz_match(fl_sz_count<SPAN>& c, uint32_t length, uint32_t distance) {
    if (SPAN) {
        if (length < 3 || length > 258 || distance < 1 || distance > 32768) return 11;
        if (c.n < distance && distance - c.n > c.need) c.need = distance - c.n;
    } else {
        if (c.n < distance || length < 3 || length > 258 || distance < 1 || distance > 32768) return 11;
    }
    c.n += length;
    return 0;
}

template <bool SPAN>
__device__ __forceinline__ int fl_sink_literal(fl_sz_count<SPAN>& c, uint32_t, uint32_t) {
    c.n++;
    return 0;
}
template <bool SPAN>
__device__ __forceinline__ int fl_sink_match(fl_sz_count<SPAN>& c, uint32_t length, uint32_t distance, uint32_t) {
    return fl_sz_match(c, fl_uni(length), fl_uni(distance));
}

// inflate.zig:89-102: LEN is added, the bytes are skipped
template <bool SPAN>
__device__ __forceinline__ int fl_sz_stored(fl_bitr& r, fl_sz_count<SPAN>& c) {
    uint32_t len;
    FL_TRY(fl_inf_stored_header(r, len));
    const uint32_t src_off = (uint32_t)fl_br_consumed(r);  // byte aligned here
    c.n += len;
    r.left -= (int64_t)len * 8;
    fl_br_seek(r, src_off + len);
    return 0;
}

// One round of a dynamic block: steps (1) and (2) of fl_inf_fast_round; the round's bytes are the sum over the chain.
// Returns 0 = go on, 1 = end of block, 2 = the next symbol needs the symbol-at-a-time path.
template <bool SPAN>
__device__ __forceinline__ int fl_sz_fast_round(fl_bitr& r, FL_LDS fl_inflate_ws16* ws, fl_sz_count<SPAN>& c, uint32_t lane) {
    const uint64_t left0 = fl_uni64((uint64_t)r.left);
    fl_round t;
    fl_round_decode(r, ws, left0, lane, t);
    fl_round_chain(t);
    const uint32_t dist = t.dist;
    const uint64_t S = t.S, m_match = t.m_match;
    uint32_t consumed = t.consumed;
    int rc = t.rc;
    // ---- (3) the round's bytes; while fewer than 32 KiB have been produced, every distance against its token's place ----
    const uint32_t mylen = FL_INV(S) ? t.olen : 0u;
    const uint32_t incl = fl_wave_incl_scan_dpp(mylen);
    uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    const uint64_t n0 = fl_uni64(c.n);
    if (__builtin_expect(n0 < 32768u, 0)) {
        const uint32_t off = incl - mylen;
        const uint64_t fm = S & m_match & FL_BALLOT(dist > (uint32_t)n0 + off);
        if (fm) {
            if (SPAN) {
                const uint32_t over = fl_wave_max(FL_INV(fm) ? dist - ((uint32_t)n0 + off) : 0u);
                if (over > c.need) c.need = over;
            } else {  // the first such token is left to the symbol-at-a-time path: InvalidMatch, in the reference's order
                const uint32_t f = (uint32_t)__builtin_ctzll(fm);
                consumed = f;
                rc = 2;
                T = (uint32_t)__builtin_amdgcn_readlane((int)off, (int)f);
            }
        }
    }
    c.n = n0 + T;
    r.left = (int64_t)(left0 - consumed);
    return rc;
}

template <bool SPAN>
__device__ __forceinline__ int fl_sz_dynamic(fl_bitr& r, FL_LDS fl_inflate_ws16* ws, fl_sz_count<SPAN>& c, uint32_t lane) {
    for (;;) {
#ifndef FL_SZ_NO_ROUNDS  // (tuning build: the symbol-at-a-time loop alone, tools/size_probe.py measures one against the other)
        if (r.left >= FL_INF_FAST_MIN_BITS) {
            int rc;
            do {
                rc = fl_sz_fast_round<SPAN>(r, ws, c, lane);
            } while (__builtin_expect(rc == 0 && r.left >= FL_INF_FAST_MIN_BITS, 1));
            fl_br_resync(r);
            if (rc == 1) return 0;
        }
#endif
        const int rc = (int)fl_uni((uint32_t)fl_inf_dynamic_symbol(r, ws, c, lane));
        if (rc < 0) return 0;
        if (rc) return rc;
    }
}

// One member from where the reader stands: the container's header (first), the blocks up to the one with BFINAL (SPAN: or
// up to the first block that starts at or behind stop_bit) and the footer, which is read, not compared.  Returns the
// status; cnt has the bytes, end_bit / final_seen what a span's record wants.  k_inflate_size counts one member with it,
// k_member_walk (kernels_members.h) one after the other.  HOOK is told every block start and the bytes counted in front
// of it (a span's stop included): the index walker's point emitter (kernels_index.h); the two kernels above tell nobody
// and compile as they did without it.  It is also told every stored block that ended well, with its LEN and BFINAL: the
// index scanner (kernels_index_scan.h) knows a flush marker by them.
struct fl_sz_no_hook {
    enum { ON = 0 };
    __device__ __forceinline__ void block_start(uint64_t, uint64_t) {}
    __device__ __forceinline__ void stored_block(uint64_t, uint32_t) {}
};
template <bool SPAN, class HOOK = fl_sz_no_hook>
__device__ __forceinline__ int fl_sz_member(fl_bitr& r, FL_LDS fl_inflate_ws16* ws, int container, int flags, uint32_t lane,
                                            bool first, uint64_t stop_bit, uint64_t total_bits, fl_sz_count<SPAN>& cnt,
                                            uint32_t& final_seen, uint64_t& end_bit, HOOK* hook = nullptr) {
    int rc = first ? (int)fl_uni((uint32_t)fl_inf_header(r, container)) : 0;
    while (rc == 0) {  // inflate.zig:251-280
        if (SPAN || HOOK::ON) {
            end_bit = total_bits - (uint64_t)r.left;  // a block starts here
            if (HOOK::ON) hook->block_start(end_bit, cnt.n);
            if (SPAN && end_bit >= stop_bit) break;
        }
        uint32_t bfinal, btype;
        if ((rc = (int)fl_uni((uint32_t)fl_br_read(r, 1, bfinal)))) break;
        if ((rc = (int)fl_uni((uint32_t)fl_br_read(r, 2, btype)))) break;
        bfinal = fl_uni(bfinal);
        btype = fl_uni(btype);
        if (btype == 2) {
            if ((rc = (int)fl_uni((uint32_t)fl_inf_dynamic_header(r, ws, flags, lane)))) break;
            rc = (int)fl_uni((uint32_t)fl_sz_dynamic<SPAN>(r, ws, cnt, lane));
        } else if (btype == 0) {
            const uint64_t n0 = HOOK::ON ? cnt.n : 0;
            rc = (int)fl_uni((uint32_t)fl_sz_stored<SPAN>(r, cnt));
            if (HOOK::ON && rc == 0) hook->stored_block(cnt.n - n0, bfinal);
        } else if (btype == 1) {
            rc = (int)fl_uni((uint32_t)fl_inf_fixed(r, cnt, lane));
        } else {
            rc = 12;  // InvalidBlockType
        }
        if (rc) break;
        if (bfinal) {
            fl_br_align(r);
            end_bit = total_bits - (uint64_t)r.left;
            // container.zig:154-166: the footer is read, not compared
            uint32_t v;
            if (container == 1) {
                if ((rc = (int)fl_uni((uint32_t)fl_br_read(r, 32, v)))) break;
                if ((rc = (int)fl_uni((uint32_t)fl_br_read(r, 32, v)))) break;
            } else if (container == 2) {
                if ((rc = (int)fl_uni((uint32_t)fl_br_read(r, 32, v)))) break;
            }
            final_seen = 1;
            break;
        }
    }
    return rc;
}

// One wave per stream (SPAN = false: workgroup i counts stream i, unless chunks[i].skip says the host has its size
// already) or per span (SPAN = true: workgroup j counts spans[j] and writes recs[j]).
#ifndef FL_SZ_WAVES
#define FL_SZ_WAVES 8  // per SIMD: 32 streams per CU, what 5 KiB of LDS each allow
#endif
template <bool SPAN>
__global__ __launch_bounds__(64, FL_SZ_WAVES) void k_inflate_size(const uint8_t* __restrict__ in, const fl_chunk* __restrict__ chunks,
                                                                   int container, int flags, uint64_t* __restrict__ sizes,
                                                                   int32_t* __restrict__ status, uint64_t* __restrict__ consumed,
                                                                   const fl_size_span* __restrict__ spans,
                                                                   fl_size_rec* __restrict__ recs) {
    __shared__ fl_inflate_ws16 ws_mem;
    __shared__ uint32_t inring_mem[FL_INF_INRING / 4];
    FL_LDS fl_inflate_ws16* ws = (FL_LDS fl_inflate_ws16*)&ws_mem;
    const uint32_t lane = threadIdx.x;
    uint32_t c = blockIdx.x;
    uint64_t start_bit = 0, stop_bit = ~0ull;
    bool first = true;
    if (SPAN) {
        const fl_size_span sp = spans[blockIdx.x];
        c = sp.stream;
        start_bit = sp.start_bit;
        stop_bit = sp.stop_bit;
        first = sp.first != 0;
    }
    const fl_chunk ck = chunks[c];
    if (!SPAN && ck.skip) return;
    fl_bitr r;
    r.data = in + ck.in_off;
    r.nbytes = ck.in_len;
    r.lane = lane;
    r.inring = (FL_LDS uint32_t*)inring_mem;
    const uint64_t total_bits = (uint64_t)ck.in_len * 8;
    r.left = (int64_t)(total_bits - (first ? 0ull : start_bit));
    fl_br_seek(r, first ? 0u : (uint32_t)(start_bit >> 3));
    if (!first) fl_br_resync(r);
    fl_sz_count<SPAN> cnt;
    cnt.n = 0;
    cnt.need = 0;
    uint32_t final_seen = 0;
    uint64_t end_bit = 0;
    const int rc = fl_sz_member<SPAN>(r, ws, container, flags, lane, first, stop_bit, total_bits, cnt, final_seen, end_bit);
    if (lane == 0) {
        if (SPAN) {
            fl_size_rec rec;
            rec.end_bit = end_bit;
            rec.out_len = cnt.n;
            rec.need_hist = cnt.need;
            rec.consumed = fl_br_consumed(r);
            rec.status = rc;
            rec.final_seen = final_seen;
            recs[blockIdx.x] = rec;
        } else {
            sizes[c] = cnt.n;
            status[c] = rc;
            if (consumed) consumed[c] = fl_br_consumed(r);
        }
    }
}
