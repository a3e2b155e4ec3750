// kernels_deflater.h -- resumable huffman-only / store-only compress (flate_hip_deflater_*): the reference's
// SimpleCompressor (deflate.zig:449-529) kept on the device between calls.  A feed stages every stream's
// buffered bytes and its new piece back to back (k_deflater_stage), the shared back end plans and packs the
// blocks that are complete (k_byte_hist, k_plan / k_plan_store, k_encode, unchanged), and two small kernels
// place those blocks behind the bits the stream already holds (k_deflater_offsets) and keep the new partial
// byte and the unfinished buffer for the next feed (k_deflater_commit).
#pragma once
#include "kernels_block.h"
#include "deflater_plan.h"

// per stream, device memory: what a SimpleCompressor carries from one write() to the next besides its buffer
struct fl_dfl_state {
    uint32_t cks_x;        // CRC-32 of the stream so far / Adler-32 sum A (zero start, mod 65521)
    uint32_t cks_y;        // Adler-32 sum B (zero start, mod 65521)
    uint64_t total;        // input bytes taken so far (ISIZE is its low 32 bits)
    uint32_t carry_byte;   // the last partial output byte, held back ...
    uint32_t carry_nbits;  // ... and how many of its bits are written (0..7)
};

// (fl_dfl_job, what the host builds per stream fed in this call: deflater_plan.h)

// buffered bytes + piece -> in[chunk.in_off ..): a grid of (jobs, slices), every thread one aligned 16-byte unit
__global__ __launch_bounds__(256) void k_deflater_stage(const uint8_t* __restrict__ src, const fl_dfl_job* __restrict__ jobs,
                                                        const fl_chunk* __restrict__ chunks, const uint8_t* __restrict__ bufs,
                                                        uint8_t* __restrict__ in) {
    const fl_dfl_job jb = jobs[blockIdx.x];
    const fl_chunk ck = chunks[blockIdx.x];
    const uint32_t L = jb.bl + jb.n;
    const uint8_t* buf = bufs + (uint64_t)jb.stream * FL_DFL_BUF;
    const uint8_t* pc = src + jb.src_off;
    uint8_t* dst = in + ck.in_off;  // 16-byte aligned, the job's region padded to 16
    const bool pc_aligned = (((uintptr_t)pc - jb.bl) & 15u) == 0;
    const uint64_t units = ((uint64_t)L + 15) >> 4;
    for (uint64_t u = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; u < units; u += (uint64_t)gridDim.y * blockDim.x) {
        const uint64_t k = u << 4;
        uint4 v;
        if (k + 16 <= jb.bl) {
            v = *(const uint4*)(buf + k);
        } else if (k >= jb.bl && k + 16 <= L && pc_aligned) {
            v = *(const uint4*)(pc + (k - jb.bl));
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < 16; t++) {
                const uint64_t x = k + t;
                const uint32_t b = x < jb.bl ? buf[x] : (x < L ? pc[x - jb.bl] : 0u);
                w[t >> 2] |= b << (8 * (t & 3));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *(uint4*)(dst + k) = v;
    }
}

// One wave per job: the header or the carried byte, the bit offset of every block behind them (the offset map of
// k_offsets, started at the carried bit), the running checksum, the footer of a finished stream, and the number of
// whole bytes this feed hands out.  Runs before k_encode, which ORs the blocks into the cleared output.
__global__ __launch_bounds__(64) void k_deflater_offsets(const fl_dfl_job* __restrict__ jobs, const fl_chunk* __restrict__ chunks,
                                                         fl_params prm, fl_crc_consts cc, fl_block_plan* __restrict__ plans,
                                                         const uint32_t* __restrict__ cks_part, fl_dfl_state* __restrict__ state,
                                                         uint8_t* __restrict__ out, uint64_t* __restrict__ produced) {
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    const fl_dfl_job jb = jobs[j];
    const fl_chunk ck = chunks[j];
    fl_dfl_state s = state[jb.stream];
    const uint32_t hdr_bytes = jb.hdr ? (prm.container == 1 ? 10u : (prm.container == 2 ? 2u : 0u)) : 0u;
    const uint32_t ftr_bytes = jb.finish ? (prm.container == 1 ? 8u : (prm.container == 2 ? 4u : 0u)) : 0u;
    const uint64_t base = (ck.out_off + hdr_bytes) * 8 + (jb.hdr ? 0u : s.carry_nbits);

    fl_offmap run;
    run.a = 0;
    run.c = 0;
    run.has = 0;
    for (uint32_t b0 = 0; b0 < ck.n_blocks; b0 += 64) {
        const uint32_t b = b0 + lane;
        fl_offmap m;
        m.a = 0;
        m.c = 0;
        m.has = 0;
        fl_block_plan* plan = b < ck.n_blocks ? &plans[ck.first_block + b] : nullptr;
        if (plan && plan->valid) {
            if (plan->type == FL_BLOCK_STORED) {
                m.a = 3;
                m.c = 32 + 8ull * plan->in_len;
                m.has = 1;
            } else {
                m.a = plan->size_bits;
            }
        }
        fl_offmap inc = m;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            fl_offmap o;
            o.a = __shfl_up(inc.a, d, 64);
            o.c = __shfl_up(inc.c, d, 64);
            o.has = __shfl_up(inc.has, d, 64);
            if (lane >= (uint32_t)d) inc = fl_offmap_compose(o, inc);
        }
        fl_offmap exc;
        exc.a = __shfl_up(inc.a, 1, 64);
        exc.c = __shfl_up(inc.c, 1, 64);
        exc.has = __shfl_up(inc.has, 1, 64);
        if (lane == 0) {
            exc.a = 0;
            exc.c = 0;
            exc.has = 0;
        }
        if (plan && plan->valid) plan->bit_off = fl_offmap_apply(fl_offmap_compose(run, exc), base);
        fl_offmap last;
        last.a = __shfl(inc.a, 63, 64);
        last.c = __shfl(inc.c, 63, 64);
        last.has = __shfl(inc.has, 63, 64);
        run = fl_offmap_compose(run, last);
    }
    const uint64_t end_bits = fl_offmap_apply(run, base);

    // the piece's checksum behind the stream's (crc(A || B) = crc(A) x^(8 |B|) + crc(B); Adler-32 sums with zero start:
    // A = A1 + A2, B = B1 + |B| A1 + B2)
    uint32_t v = 0;
    if (prm.container != 0) v = fl_fold_checksums(cks_part, jb.ck_first, jb.ck_n, prm.container, cc, lane);
    if (lane != 0) return;
    if (prm.container == 1) {
        s.cks_x = fl_crc_mulmod(s.cks_x, fl_crc_xpow8n(cc.xpow8, jb.n)) ^ v;
    } else if (prm.container == 2) {
        const uint32_t nm = jb.n % 65521u;
        const uint32_t pa = ((v & 0xffffu) + 65520u) % 65521u, pb = ((v >> 16) + 65521u - nm) % 65521u;
        s.cks_y = (uint32_t)(((uint64_t)s.cks_y + (uint64_t)nm * s.cks_x + pb) % 65521u);
        s.cks_x = (s.cks_x + pa) % 65521u;
    }
    s.total += jb.n;

    uint8_t* o = out + ck.out_off;
    if (jb.hdr) {
        if (prm.container == 1) {  // container.zig:64
            const uint8_t h[10] = {0x1f, 0x8b, 0x08, 0, 0, 0, 0, 0, 0, 0x03};
            for (int i = 0; i < 10; i++) o[i] = h[i];
        } else if (prm.container == 2) {
            o[0] = 0x78;
            o[1] = 0x9c;
        }
    } else if (s.carry_nbits) {
        o[0] = (uint8_t)s.carry_byte;
    }
    uint64_t n_out;
    if (jb.finish) {
        const uint64_t body_end = (end_bits + 7) >> 3;  // bit_writer.flush pads the last byte
        uint8_t* f = out + body_end;
        if (prm.container == 1) {  // container.zig:92-96
            for (int i = 0; i < 4; i++) f[i] = (uint8_t)(s.cks_x >> (8 * i));
            for (int i = 0; i < 4; i++) f[4 + i] = (uint8_t)(s.total >> (8 * i));
        } else if (prm.container == 2) {  // container.zig:104
            const uint32_t a = (1u + s.cks_x) % 65521u;
            const uint32_t b = (uint32_t)((s.total % 65521u + s.cks_y) % 65521u);
            const uint32_t c = a | (b << 16);
            for (int i = 0; i < 4; i++) f[i] = (uint8_t)(c >> (8 * (3 - i)));
        }
        n_out = body_end + ftr_bytes - ck.out_off;
        s.carry_nbits = 0;
    } else {
        n_out = (end_bits >> 3) - ck.out_off;
        s.carry_nbits = (uint32_t)(end_bits & 7);
    }
    s.carry_byte = 0;
    produced[j] = n_out;
    state[jb.stream] = s;
}

// After k_encode: the partial last byte is held back for the next feed, and the tail of the staged input that no
// block took goes back into the stream's buffer.
__global__ __launch_bounds__(256) void k_deflater_commit(const fl_dfl_job* __restrict__ jobs, const fl_chunk* __restrict__ chunks,
                                                         const uint64_t* __restrict__ produced, const uint8_t* __restrict__ in,
                                                         const uint8_t* __restrict__ out, fl_dfl_state* __restrict__ state,
                                                         uint8_t* __restrict__ bufs) {
    const uint32_t j = blockIdx.x;
    const fl_dfl_job jb = jobs[j];
    const fl_chunk ck = chunks[j];
    if (threadIdx.x == 0 && state[jb.stream].carry_nbits) state[jb.stream].carry_byte = out[ck.out_off + produced[j]];
    const uint8_t* src = in + ck.in_off + (jb.bl + jb.n - jb.keep);
    uint8_t* dst = bufs + (uint64_t)jb.stream * FL_DFL_BUF;
    for (uint32_t k = threadIdx.x; k < jb.keep; k += blockDim.x) dst[k] = src[k];
}
