// kernels_inflate_size.h -- the size probe (flate_hip_decompressed_sizes): how many bytes a stream inflates to, without
// inflating it.  One wavefront per stream, or per span of a long stream (size_plan.h).
//
// Bit reader, container header, dynamic block header with its table build and the fixed code are those of
// kernels_inflate.h, called as they are; the decode loops are new.  A literal adds 1 to a 64-bit counter, a match its
// length after the checks of fl_inf_match, a stored block its LEN.  Nothing is produced: no output ring, no flush, no
// store except the three result words, and the footer is read but not compared (there are no bytes to sum).  What a
// stream keeps in LDS is the decoder tables and the staged input, 5 KiB: 32 streams per CU instead of k_inflate's 20.
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

// inflate.zig:89-102: LEN is added, the bytes are skipped
template <bool SPAN>
__device__ __forceinline__ int fl_sz_stored(fl_bitr& r, fl_sz_count<SPAN>& c) {
    fl_br_align(r);
    uint32_t len, nlen;
    FL_TRY(fl_br_read(r, 16, len));
    FL_TRY(fl_br_read(r, 16, nlen));
    len = fl_uni(len);
    nlen = fl_uni(nlen);
    if (len != ((~nlen) & 0xffff)) return 13;
    if ((int64_t)len * 8 > r.left) return 1;
    const uint32_t src_off = (uint32_t)fl_br_consumed(r);  // byte aligned here
    c.n += len;
    r.left -= (int64_t)len * 8;
    fl_br_seek(r, src_off + len);
    return 0;
}

// bit_reader.zig:205-217 + inflate.zig:104-121 (fl_inf_fixed's loop with the counter in the output's place)
template <bool SPAN>
__device__ __forceinline__ int fl_sz_fixed(fl_bitr& r, fl_sz_count<SPAN>& c) {
    for (;;) {
        FL_TRY(fl_br_fill(r, 9));
        const uint32_t code7 = fl_uni(fl_rev_bits(fl_br_peek(r, 7), 7));
        FL_TRY(fl_br_shift(r, 7));
        uint32_t code;
        if (code7 <= 0x17) {
            code = code7 + 256;
        } else if (code7 <= 0x5f) {
            const uint32_t e = fl_br_peek(r, 1);
            FL_TRY(fl_br_shift(r, 1));
            code = (code7 << 1) + e - 0x30;
        } else if (code7 <= 0x63) {
            const uint32_t e = fl_br_peek(r, 1);
            FL_TRY(fl_br_shift(r, 1));
            code = ((code7 - 0x60) << 1) + e + 280;
        } else {
            const uint32_t e = fl_rev_bits(fl_br_peek(r, 2), 2);
            FL_TRY(fl_br_shift(r, 2));
            code = ((code7 - 0x64) << 2) + e + 144;
        }
        code = fl_uni(code);
        if (code <= 255) {
            c.n++;
        } else if (code == 256) {
            return 0;
        } else if (code <= 285) {
            FL_TRY(fl_br_fill(r, 5 + 5 + 13));
            uint32_t length, distance;
            FL_TRY(fl_inf_length(r, code - 257, length));
            const uint32_t dcode = fl_rev_bits(fl_br_peek(r, 5), 5);
            FL_TRY(fl_br_shift(r, 5));
            FL_TRY(fl_inf_distance(r, dcode, distance));
            FL_TRY(fl_sz_match(c, fl_uni(length), fl_uni(distance)));
        } else {
            return 7;
        }
    }
}

// one symbol of a dynamic block (fl_inf_dynamic_symbol with the counter in the output's place); -1 at the end of the block
template <bool SPAN>
__device__ __forceinline__ int fl_sz_dynamic_symbol(fl_bitr& r, FL_LDS fl_inflate_ws16* ws, fl_sz_count<SPAN>& c) {
    FL_TRY(fl_br_fill(r, 15));
    uint32_t sym, cb;
    {
        const uint32_t pk = fl_br_peek(r, 15);
        const uint32_t e = fl_uni(ws->lit_lut[pk & ((1u << FL_INF_LIT_BITS) - 1)]);
        if (e) {
            sym = e & 0x1ff;
            cb = (e >> 9) & 15;
        } else {
            FL_TRY(fl_hdec_find(&ws->lit, pk, 15, sym, cb));
            sym = fl_uni(sym);
            cb = fl_uni(cb);
        }
    }
    FL_TRY(fl_br_shift(r, cb));
    if (sym < 256) {
        c.n++;
    } else if (sym == 256) {
        return -1;
    } else {
        FL_TRY(fl_br_fill(r, 5 + 15 + 13));
        uint32_t length, distance, dsym;
        FL_TRY(fl_inf_length(r, sym - 257, length));
        {
            const uint32_t pk = fl_br_peek(r, 15);
            const uint16_t e = (uint16_t)fl_uni(ws->dst_lut[pk & ((1u << FL_INF16_DST_BITS) - 1)]);
            if (e) {
                fl_dst_sym_cb(e, dsym, cb);
            } else {
                FL_TRY(fl_hdec_find(&ws->dst, pk, 15, dsym, cb));
                dsym = fl_uni(dsym);
                cb = fl_uni(cb);
            }
        }
        FL_TRY(fl_br_shift(r, cb));
        FL_TRY(fl_inf_distance(r, dsym, distance));
        FL_TRY(fl_sz_match(c, fl_uni(length), fl_uni(distance)));
    }
    return 0;
}

// One round of a dynamic block: steps (1) to (3) of fl_inf_fast_round, whose comments say why they are written as they
// are; the round's bytes are the sum over the chain.  Returns 0 = go on, 1 = end of block, 2 = the next symbol needs the
// symbol-at-a-time path.
template <bool SPAN>
__device__ __forceinline__ int fl_sz_fast_round(fl_bitr& r, FL_LDS fl_inflate_ws16* ws, fl_sz_count<SPAN>& c, uint32_t lane) {
    const uint64_t left0 = fl_uni64((uint64_t)r.left);
    const uint64_t pos = (uint64_t)fl_uni(r.nbytes) * 8 - left0;
    const uint32_t byte0 = (uint32_t)(pos >> 3);
    if (__builtin_expect(byte0 + 24 > fl_uni(r.in_loaded), 0)) fl_br_commit_half(r);
    // ---- (1) the token that starts at pos + lane ----
    const uint32_t bp = ((byte0 & (FL_INF_INRING - 1)) << 3) + ((uint32_t)pos & 7) + lane;  // bit index in the ring
    const uint32_t di = bp >> 5;
    const uint32_t IM = FL_INF_INRING / 4 - 1;
    const uint32_t d0 = r.inring[di & IM], d1 = r.inring[(di + 1) & IM], d2 = r.inring[(di + 2) & IM];
    const uint32_t w0 = __builtin_amdgcn_alignbit(d1, d0, bp & 31);  // stream bits [pos + lane, + 32)
    const uint32_t w1 = __builtin_amdgcn_alignbit(d2, d1, bp & 31);  // ... [+ 32, + 64)
    const uint32_t le = ws->lit_lut[w0 & ((1u << FL_INF_LIT_BITS) - 1)];
    const uint32_t lsym = le & 511, lcb = (le >> 9) & 15, leb = le >> 13;
    const uint64_t m_lok = FL_BALLOT(le != 0) & FL_BALLOT(leb != 7);
    const uint64_t m_lit = m_lok & FL_BALLOT(lsym < 256);
    const uint32_t lbits = lcb + leb;  // at most 10 + 5
    const uint32_t wd = __builtin_amdgcn_alignbit(w1, w0, lbits & 31);  // the 32 bits behind the length code
    const uint32_t de = ws->dst_lut[wd & ((1u << FL_INF16_DST_BITS) - 1)];
    const uint32_t dsym = de & 31, dcb = (de >> 5) & 15, deb = de >> 9;
    const uint64_t m_match = m_lok & FL_BALLOT(lsym > 256) & FL_BALLOT(de != 0) & FL_BALLOT(deb != 15);
    const uint64_t m_plain = m_lit | m_match;
    const bool is_lit = FL_INV(m_lit), is_match = FL_INV(m_match);
    const uint32_t lc = lsym - 257;
    uint32_t lbase = ((4u | (lc & 3u)) << leb) + 3u;
    lbase = FL_INV(FL_BALLOT(leb != 0)) ? lbase : lc + 3u;
    lbase = FL_INV(FL_BALLOT(lc == 28u)) ? 258u : lbase;
    uint32_t dbase = ((2u | (dsym & 1u)) << deb) + 1u;
    dbase = FL_INV(FL_BALLOT(deb != 0)) ? dbase : dsym + 1u;
    const uint32_t length = lbase + ((w0 >> lcb) & ((1u << leb) - 1));
    const uint32_t dist = dbase + ((wd >> dcb) & ((1u << deb) - 1));
    // anything that is not a plain literal or match ends the chain: it is the last member of S
    const uint32_t nb = is_lit ? lcb : is_match ? lbits + dcb + deb : 64u;
    const uint32_t olen = is_lit ? 1u : is_match ? length : 0u;
    // ---- (2) the chain of token starts ----
    uint64_t S = 0;
    uint32_t p = 0u - 64u, pn;
    asm volatile(
        "1:\n\t"
        "s_bitset1_b64 %[S], %[p]\n\t"
        "v_readlane_b32 %[n], %[nb], %[p]\n\t"
        "s_add_u32 %[p], %[p], %[n]\n\t"
        "s_cbranch_scc0 1b\n\t"
        : [S] "+s"(S), [p] "+s"(p), [n] "=&s"(pn)
        : [nb] "v"(nb)
        : "scc");
    p += 64u;
    int rc = 0;
    uint32_t consumed = p;
    {
        const uint32_t top = 63u - (uint32_t)__builtin_clzll(S);
        if (__builtin_expect(!((m_plain >> top) & 1), 0)) {
            if (((m_lok & FL_BALLOT(lsym == 256)) >> top) & 1) {
                consumed = top + (uint32_t)__builtin_amdgcn_readlane((int)lcb, (int)top);
                rc = 1;
            } else {
                consumed = top;
                rc = 2;
            }
        }
    }
    // ---- (3) the round's bytes; while fewer than 32 KiB have been produced, every distance against its token's place ----
    const uint32_t mylen = FL_INV(S) ? olen : 0u;
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
        const int rc = (int)fl_uni((uint32_t)fl_sz_dynamic_symbol<SPAN>(r, ws, c));
        if (rc < 0) return 0;
        if (rc) return rc;
    }
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

    int rc = first ? (int)fl_uni((uint32_t)fl_inf_header(r, container)) : 0;
    while (rc == 0) {  // inflate.zig:251-280
        if (SPAN) {
            end_bit = total_bits - (uint64_t)r.left;  // a block starts here
            if (end_bit >= stop_bit) break;
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
            rc = (int)fl_uni((uint32_t)fl_sz_stored<SPAN>(r, cnt));
        } else if (btype == 1) {
            rc = (int)fl_uni((uint32_t)fl_sz_fixed<SPAN>(r, cnt));
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
