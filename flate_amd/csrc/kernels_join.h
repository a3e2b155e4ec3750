// kernels_join.h -- flate_hip_compress_joined (join_plan.h: what the bytes are and every host decision): the pieces of a
// call are raw chunk-path streams in scratch slots; k_join_open turns every piece that is not its stream's last into what
// a fresh reference compressor has written after write(piece); flush(), k_join_scan gives every piece its place in its
// stream's slot and folds the stream's checksum and status, k_join_pack copies the pieces there and writes header and footer.
// All three are bound by memory or trivially small: nothing here computes.
#pragma once
#include <hip/hip_runtime.h>

#include "join_plan.h"
#include "kernels_block.h"
#include "kernels_common.h"

// Behind a chunk-path pass's back end, while its plans hold the pass's blocks: a thread per piece of the pass.  The last
// valid plan of the piece's chunk says where the final block's first header bit (BFINAL) lies and at which bit the block ends
// (a stored block ends on a byte boundary).  A piece that is not its stream's last: that bit is cleared, the marker is
// written out byte by byte behind the piece (slot bytes beyond out_len are unspecified) and counted into its length.
// Every piece: its checksum part (k_checksum's, when the container has one) leaves the pass's workspace.
// c0: the pass's first piece among the call's pieces; piece_len / piece_status / piece_cks are the call's arrays.
__global__ __launch_bounds__(256) void k_join_open(const fl_chunk* __restrict__ chunks, const fl_block_plan* __restrict__ plans,
                                                   uint32_t nc, uint32_t c0, const uint32_t* __restrict__ piece_stream,
                                                   const fl_join_stream* __restrict__ streams, uint8_t* __restrict__ scratch,
                                                   uint64_t* __restrict__ piece_len, int32_t* __restrict__ piece_status,
                                                   const uint32_t* __restrict__ cks_part, uint32_t* __restrict__ piece_cks) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nc) return;
    const uint64_t j = (uint64_t)c0 + i;
    const uint32_t first_block = chunks[i].first_block, n_blocks = chunks[i].n_blocks;
    if (cks_part) piece_cks[j] = cks_part[2 * (uint64_t)first_block];
    const fl_join_stream& s = streams[piece_stream[j]];
    if (j + 1 == s.piece0 + s.n_pieces) return;  // the stream's last piece
    const uint64_t len = piece_len[j];
    if (piece_status[j] == 100 || len == 0) return;  // (its slot holds a bound: never)
    const fl_block_plan* last = nullptr;
    for (uint32_t b = n_blocks; b > 0 && !last; b--)
        if (plans[first_block + b - 1].valid) last = &plans[first_block + b - 1];
    if (!last) return;
    const uint64_t bit = last->bit_off;
    const uint64_t end = last->type == FL_BLOCK_STORED ? ((bit + 3 + 7) & ~7ull) + 32 + 8ull * last->in_len : bit + last->size_bits;
    const uint32_t m = fl_join_marker_bytes((uint32_t)(end & 7u));
    const uint64_t slot = chunks[i].out_off, cap = chunks[i].out_cap;
    if (len + m > cap || ((end + 7) >> 3) != slot + len) {  // (never: the slot holds the bound and the marker)
        piece_status[j] = 100;
        return;
    }
    scratch[bit >> 3] &= (uint8_t)~(1u << (bit & 7u));
    uint8_t* p = scratch + slot + len;
    if (m == 5) *p++ = 0;
    p[0] = 0;
    p[1] = 0;
    p[2] = 0xff;
    p[3] = 0xff;
    piece_len[j] = len + m;
}

// A workgroup per stream, over its pieces 256 at a time: the running sum of their lengths gives every piece its place
// behind the container header (piece_dst: an offset into `out`); the first non-zero piece status is the stream's.  Then the
// pieces' checksum parts: every thread folds a run of consecutive pieces (Horner: one polynomial product per piece, and all
// pieces but the last are `piece` bytes: one power), moves its result to the end of the stream -- crc(A || B) =
// crc(A) x^(8 |B|) + crc(B), Adler-32: A = sum of the A's, B = sum of (B + A * bytes behind); the bytes behind a run need no
// scan -- and the results are added up.  Then out_len and status of the stream (100: it does not fit its slot, nothing is
// written) and its checksum for k_join_pack.
__global__ __launch_bounds__(256) void k_join_scan(const fl_join_stream* __restrict__ streams, uint32_t piece, int container,
                                                   fl_crc_consts cc, const uint64_t* __restrict__ piece_len,
                                                   const int32_t* __restrict__ piece_status, const uint32_t* __restrict__ piece_cks,
                                                   uint64_t* __restrict__ piece_dst, uint64_t* __restrict__ out_len,
                                                   int32_t* __restrict__ status, uint32_t* __restrict__ stream_cks) {
    __shared__ uint64_t wsum[4];
    __shared__ uint64_t carry;
    __shared__ uint32_t first_bad;
    __shared__ uint32_t wx[4], wy[4];
    const fl_join_stream s = streams[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t hdr = container == 1 ? 10u : (container == 2 ? 2u : 0u);
    const uint32_t ftr = container == 1 ? 8u : (container == 2 ? 4u : 0u);
    if (tid == 0) {
        carry = 0;
        first_bad = 0xffffffffu;
    }
    __syncthreads();
    for (uint64_t base = 0; base < s.n_pieces; base += 256) {
        const uint64_t k = base + tid;
        const bool have = k < s.n_pieces;
        const uint64_t v = have ? piece_len[s.piece0 + k] : 0;
        uint64_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t t = __shfl_up(inc, d, 64);
            if (lane >= (uint32_t)d) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint64_t off = carry;
        for (uint32_t w = 0; w < wave; w++) off += wsum[w];
        if (have) {
            piece_dst[s.piece0 + k] = s.out_off + hdr + off + inc - v;
            if (piece_status[s.piece0 + k] != 0) atomicMin(&first_bad, (uint32_t)k);
        }
        __syncthreads();
        if (tid == 255) carry = off + inc;
        __syncthreads();
    }
    uint32_t x = 0, y = 0;  // crc | (A, B) of this thread's run of pieces, then moved to the end of the stream
    if (container != 0) {
        const uint64_t per = (s.n_pieces + 255) / 256;
        const uint64_t k0 = min((uint64_t)tid * per, s.n_pieces), k1 = min(k0 + per, s.n_pieces);
        const uint32_t last_len = (uint32_t)(s.n - (s.n_pieces - 1) * piece);
        const uint32_t xp = container == 1 && k1 > k0 ? (piece == FL_BLOCK_BYTES ? cc.pow65535 : fl_crc_xpow8n(cc.xpow8, piece)) : 0u;
        for (uint64_t k = k0; k < k1; k++) {
            const uint32_t pc = piece_cks[s.piece0 + k];
            const uint32_t len = k + 1 == s.n_pieces ? last_len : piece;
            if (container == 1) {
                x = fl_crc_mulmod(x, len == piece ? xp : fl_crc_xpow8n(cc.xpow8, len)) ^ pc;
            } else {
                y = (uint32_t)(((uint64_t)y + (uint64_t)x * len + (pc >> 16)) % 65521u);
                x = (x + (pc & 0xffffu)) % 65521u;
            }
        }
        const uint64_t e = k1 * piece;
        const uint64_t behind = e < s.n ? s.n - e : 0;
        if (container == 1)
            x = k1 > k0 ? fl_crc_mulmod(x, fl_crc_xpow8n(cc.xpow8, behind)) : 0u;
        else
            y = (uint32_t)(((uint64_t)y + (uint64_t)x * (behind % 65521u)) % 65521u);
    }
    uint32_t px, py = 0;
    if (container == 1) {
        px = fl_wave_xor(x);
    } else {
        px = fl_wave_sum(x);  // (64 terms below 65521 each)
        py = fl_wave_sum(y);
    }
    if (lane == 0) {
        wx[wave] = px;
        wy[wave] = py;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t fx = 0, fy = 0;
        for (uint32_t w = 0; w < 4; w++) {
            if (container == 1) {
                fx ^= wx[w];
            } else {
                fx = (fx + wx[w]) % 65521u;
                fy = (fy + wy[w]) % 65521u;
            }
        }
        // Adler-32: a = 1 + A, b = n + B
        stream_cks[blockIdx.x] = container == 1 ? fx : (((1u + fx) % 65521u) | ((uint32_t)((s.n % 65521u + fy) % 65521u) << 16));
        const uint64_t total = hdr + carry + ftr;
        const bool fits = total <= s.out_cap;
        out_len[blockIdx.x] = fits ? total : 0;
        status[blockIdx.x] = fits ? (first_bad != 0xffffffffu ? piece_status[s.piece0 + first_bad] : 0) : 100;
    }
}

// gridDim.y workgroups per piece (fl_gather_one: 16-byte stores, the unaligned edges byte by byte): the piece goes from
// its scratch slot to its place in its stream's slot, unless the stream does not fit (status 100: its slot is not
// touched).  The workgroup of a stream's first piece writes the container's header and footer (container.zig:64, 78,
// 92-96, 104): CRC-32 and the length mod 2^32, or the big-endian Adler-32, of the WHOLE stream.  Every byte written lies in
// [out_off, out_off + out_len) of its stream.
__global__ __launch_bounds__(256) void k_join_pack(const uint8_t* __restrict__ scratch, const uint64_t* __restrict__ piece_slot,
                                                   const uint64_t* __restrict__ piece_len, const uint64_t* __restrict__ piece_dst,
                                                   const uint32_t* __restrict__ piece_stream,
                                                   const fl_join_stream* __restrict__ streams, int container,
                                                   const uint64_t* __restrict__ out_len, const int32_t* __restrict__ status,
                                                   const uint32_t* __restrict__ stream_cks, uint8_t* __restrict__ out) {
    const uint32_t j = blockIdx.x, si = piece_stream[j];
    if (status[si] == 100) return;
    fl_gather_one(scratch, piece_slot, piece_len, out, piece_dst, j, blockIdx.y, gridDim.y);
    if (container == 0 || blockIdx.y != 0 || threadIdx.x != 0) return;
    const fl_join_stream& s = streams[si];
    if (j != s.piece0) return;
    uint8_t* o = out + s.out_off;
    const uint32_t cks = stream_cks[si];
    if (container == 1) {
        const uint8_t h[10] = {0x1f, 0x8b, 0x08, 0, 0, 0, 0, 0, 0, 0x03};
        for (int i = 0; i < 10; i++) o[i] = h[i];
        uint8_t* f = o + out_len[si] - 8;
        for (int i = 0; i < 4; i++) f[i] = (uint8_t)(cks >> (8 * i));
        for (int i = 0; i < 4; i++) f[4 + i] = (uint8_t)((uint32_t)s.n >> (8 * i));
    } else {
        o[0] = 0x78;
        o[1] = 0x9c;
        uint8_t* f = o + out_len[si] - 4;
        for (int i = 0; i < 4; i++) f[i] = (uint8_t)(cks >> (8 * (3 - i)));
    }
}
