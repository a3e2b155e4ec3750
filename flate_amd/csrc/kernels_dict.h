// kernels_dict.h -- compressing against preset dictionaries (flate_hip_compress_batch_dict): the staging kernel that
// writes a stream's history and record side by side for the whole-stream pass, and the header of a zlib stream with
// FDICT.  (dict_compress_plan.h: the layout and why; the tokenizer's part is fl_chunk::hist, kernels_parse.h / stream_tables.h)
#pragma once
#include "dict_compress_plan.h"
#include "dict_plan.h"
#include "kernels_common.h"

#define FL_DSTG_THREADS 256

// 16 bytes from p, whatever its alignment, by aligned 16-byte loads: the granule that holds p[0] and, when p is not
// aligned and more than 16 - (p & 15) bytes are wanted, the one behind it.  `want` (1..16) bytes of the result count.
__device__ __forceinline__ uint4 fl_dstg_load16(const uint8_t* p, uint32_t want) {
    const uint32_t sh = (uint32_t)((uintptr_t)p & 15);
    const uint4* g = (const uint4*)(p - sh);
    const uint4 a = g[0];
    if (sh == 0) return a;
    uint4 b = make_uint4(0, 0, 0, 0);
    if (want > 16u - sh) b = g[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t d = sh >> 2, bsh = sh & 3u;
    uint32_t r[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        // (d + k + 1 <= 7: d <= 3)
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            if (d == s) {
                lo = w[s + k];
                hi = w[s + k + 1];
            }
        }
        r[k] = __builtin_amdgcn_alignbyte(hi, lo, bsh);
    }
    return make_uint4(r[0], r[1], r[2], r[3]);
}

// One workgroup per staged stream: stage[dst, dst + hist + n) = dict[tsrc, tsrc + hist) ++ in[src, src + n), zeros up
// to the next multiple of 16.  dst is a multiple of 16: every store is a whole aligned granule; a granule that lies in
// the history or in the record alone is one (or two) 16-byte loads, the one across the seam and the last one are put
// together byte by byte.  Thousands of workgroups read one shared dictionary: it stays in L2.
__global__ __launch_bounds__(FL_DSTG_THREADS) void k_dict_stage(const uint8_t* __restrict__ in, const uint8_t* __restrict__ dict,
                                                                 const fl_dictc_job* __restrict__ jobs, uint8_t* __restrict__ stage) {
    const fl_dictc_job jb = jobs[blockIdx.x];
    const uint32_t D = jb.hist, total = jb.hist + jb.n;
    const uint8_t* t = dict + jb.tsrc;
    const uint8_t* r = in + jb.src;
    uint4* out = (uint4*)(stage + jb.dst);
    const uint32_t ngran = (total + 15u) >> 4;
    for (uint32_t g = threadIdx.x; g < ngran; g += FL_DSTG_THREADS) {
        const uint32_t b0 = 16u * g, b1 = min(b0 + 16u, total);
        uint4 v;
        if (b1 <= D) {
            v = fl_dstg_load16(t + b0, b1 - b0);
        } else if (b0 >= D && b1 == b0 + 16u) {
            v = fl_dstg_load16(r + (b0 - D), 16u);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t b = b0; b < b1; b++) {
                const uint32_t x = b < D ? t[b] : r[b - D];
                w[(b - b0) >> 2] |= x << (8u * (b & 3u));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        out[g] = v;
    }
}

// The header of a zlib stream with a preset dictionary, a thread per staged stream, behind the back end: CMF 78, FLG bb
// (the reference's 9c with FDICT set and FCHECK made good), the DICTID -- the Adler-32 of the WHOLE dictionary, big
// endian (k_dict_adler) -- in place of the header the back end wrote four bytes into the slot (chunks[i].out_off is
// where that one lies), and the four bytes counted.  A stream that did not fit is left alone.
__global__ __launch_bounds__(64) void k_dict_header(const fl_chunk* __restrict__ chunks, const fl_dictc_job* __restrict__ jobs,
                                                    uint32_t n, const fl_dict_ent* __restrict__ tab, uint8_t* __restrict__ out,
                                                    uint64_t* __restrict__ out_len, const int32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n || status[i] == 100) return;
    const uint32_t id = tab[jobs[i].dict].adler;
    uint8_t* o = out + chunks[i].out_off - 4;
    o[0] = 0x78;
    o[1] = 0xbb;
    for (int k = 0; k < 4; k++) o[2 + k] = (uint8_t)(id >> (8 * (3 - k)));
    out_len[i] += 4;
}
