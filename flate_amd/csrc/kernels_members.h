// kernels_members.h -- flate_hip_decompress_members: where the members of concatenated streams start, found on the device.
//
// Both ways end in a member table: per stream the start (relative to the stream) and the probed size of every member on
// its chain and, where the walk stopped on an error or at a byte no member can start at, one last entry for the failing
// remainder.  The decode that follows (the batch decoder over the members as streams of their own) has the last word on
// every status; the table only says where to cut.
//
//   scan (gzip)   k_member_scan finds every 1f 8b 08 inside a stream (count, exclusive scan, fill: the list is sized from
//                 the count), each becomes a chunk "from here to the end of the stream" that k_inflate_size<false>
//                 probes as it stands, one wave each, and k_member_chain follows each stream's chain of successors
//                 (member_plan.h).  False candidates -- the magic inside compressed bits, a stored block, an FNAME -- are
//                 probed and never reached.
//   walk          k_member_walk, one wave per stream: fl_sz_member in a loop.  zlib and raw cannot be speculated (a zlib
//                 header is 2 bytes that 1 byte in 32 satisfies, raw has none); gzip takes it when told to or when a
//                 call has too many candidates.  Always correct, only slow: a file is walked by one wave.
//
// k_member_pack puts the tables back to back for the host, k_member_fold folds the members' results into the streams'.
#pragma once
#include "kernels_inflate_size.h"
#include "member_plan.h"

// One wave per FL_MEM_SCAN_TILE bytes of the batch's input [lo, hi): 16 steps of 16 bytes a lane (a 16-byte load at a
// 16-byte aligned address, the 2 bytes behind it from the dword that follows).  `rel0` is where tile 0 starts relative to
// `in`: at or below lo, so that in + rel0 is 16-byte aligned (a load may begin in front of lo or end behind hi, inside the
// aligned 16 bytes that hold a byte of the input; what lies outside is not looked at).  A match counts when its three
// bytes lie inside ONE stream.  FILL = false: tiles[t] = matches of tile t.  FILL = true: tiles[] is the exclusive scan
// of those counts; the matches go to cand_pos[] in ascending order -- tiles ascend, steps ascend, lanes ascend -- with
// their chunks (n_cand of them: what the count found).
template <bool FILL>
__global__ __launch_bounds__(64) void k_member_scan(const uint8_t* __restrict__ in, int64_t rel0, uint64_t lo, uint64_t hi,
                                                    const uint64_t* __restrict__ in_off, uint32_t n_streams,
                                                    uint64_t* __restrict__ tiles, uint64_t* __restrict__ cand_pos,
                                                    fl_chunk* __restrict__ chunks, uint64_t n_cand) {
    const uint32_t lane = threadIdx.x;
    const int64_t t0 = rel0 + (int64_t)blockIdx.x * (int64_t)FL_MEM_SCAN_TILE;
    const uint64_t base = FILL ? tiles[blockIdx.x] : 0;
    uint32_t total = 0;
#pragma unroll 4
    for (uint32_t step = 0; step < FL_MEM_SCAN_TILE / 1024u; step++) {
        const int64_t p0 = t0 + (int64_t)(step * 1024u + lane * 16u);
        uint32_t w[5] = {0, 0, 0, 0, 0};
        if (p0 + 16 > (int64_t)lo && p0 < (int64_t)hi) {
            const uint4 v = *(const uint4*)(in + p0);
            w[0] = v.x;
            w[1] = v.y;
            w[2] = v.z;
            w[3] = v.w;
            if (p0 + 16 < (int64_t)hi) w[4] = *(const uint32_t*)(in + p0 + 16);
        }
        uint32_t m = 0;
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) {
            const uint32_t win = __builtin_amdgcn_alignbyte(w[b / 4 + 1], w[b / 4], b & 3) & 0xffffffu;
            m |= (win == 0x088b1fu ? 1u : 0u) << b;
        }
        if (!FL_BALLOT(m != 0)) continue;
        // (rare from here on: a member start, or three bytes in 16 Mi of anything else)
        uint32_t valid = 0;
        for (uint32_t b = 0; b < 16; b++) {
            if (!((m >> b) & 1)) continue;
            const int64_t p = p0 + (int64_t)b;
            if (p < (int64_t)lo || (uint64_t)p + 3 > hi) continue;
            const uint32_t s = fl_member_stream_of(in_off, n_streams, (uint64_t)p);
            if ((uint64_t)p + 3 <= in_off[s + 1]) valid |= 1u << b;
        }
        const uint32_t cnt = (uint32_t)__builtin_popcount(valid);
        const uint32_t incl = fl_wave_incl_scan_dpp(cnt);
        if (FILL) {
            uint64_t at = base + total + incl - cnt;
            for (uint32_t b = 0; b < 16; b++) {
                if (!((valid >> b) & 1)) continue;
                const uint64_t p = (uint64_t)(p0 + (int64_t)b);
                fl_chunk c{};
                c.in_off = p;
                c.in_len = (uint32_t)(in_off[fl_member_stream_of(in_off, n_streams, p) + 1] - p);
                if (at < n_cand) {  // (the count was taken from these bytes: always, unless they changed since)
                    cand_pos[at] = p;
                    chunks[at] = c;
                }
                at++;
            }
        }
        total += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (!FILL && lane == 0) tiles[blockIdx.x] = total;
}

// One wave per stream: the stream's candidates are cand_pos[lo_c .. hi_c) (the list is ascending over the whole batch);
// every candidate's successor in parallel, then the chain from the stream's first byte (fl_member_follow).  The stream's
// table goes to entries [lo_c + s ..): at most its candidates and one failing remainder.
__global__ __launch_bounds__(64) void k_member_chain(const uint64_t* __restrict__ in_off, const uint64_t* __restrict__ cand_pos,
                                                     uint32_t n_cand, const int32_t* __restrict__ p_status,
                                                     const uint64_t* __restrict__ p_consumed, const uint64_t* __restrict__ p_size,
                                                     uint32_t* __restrict__ succ, uint32_t* __restrict__ chain,
                                                     uint64_t* __restrict__ tab_off, uint64_t* __restrict__ tab_n,
                                                     uint32_t* __restrict__ tab_start, uint64_t* __restrict__ tab_size,
                                                     uint64_t* __restrict__ n_on) {
    __shared__ uint32_t tile[FL_MEM_LDS_TILE];
    __shared__ uint32_t stop_mem;
    const uint32_t lane = threadIdx.x, s = blockIdx.x;
    const uint64_t a = in_off[s], e = in_off[s + 1];
    const uint32_t lo_c = fl_member_lower_bound(cand_pos, n_cand, a);
    const uint32_t nc = fl_member_lower_bound(cand_pos + lo_c, n_cand - lo_c, e);
    const uint64_t* pos = cand_pos + lo_c;
    for (uint32_t i = lane; i < nc; i += 64)
        succ[lo_c + i] = fl_member_successor(pos, nc, i, p_status[lo_c + i], p_consumed[lo_c + i], e);
    __syncthreads();
    const uint32_t first = nc && pos[0] == a ? 0u : FL_MEM_MISS;
    const uint32_t count = fl_member_follow(
        succ + lo_c, nc, first, tile, lane, 64u, [] { __syncthreads(); }, [](uint32_t v) { return fl_uni(v); }, chain + lo_c,
        &stop_mem);
    __syncthreads();
    const uint32_t stop = stop_mem;
    const uint64_t base = (uint64_t)lo_c + s;
    const uint32_t m = fl_member_table(chain + lo_c, count, stop, pos, p_consumed + lo_c, p_size + lo_c, a, lane, 64u,
                                       tab_start + base, tab_size + base);
    if (lane == 0) {
        tab_off[s] = base;
        tab_n[s] = m;
        n_on[s] = count;
    }
}

// One wave per stream: member after member from the stream's first byte, each as k_inflate_size<false> counts it.  The
// stream's table is entries [tab_off[s], tab_off[s + 1]): the host sized it by fl_member_least_bytes.
__global__ __launch_bounds__(64, FL_SZ_WAVES) void k_member_walk(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                                  int container, int flags, const uint64_t* __restrict__ tab_off,
                                                                  uint64_t* __restrict__ tab_n, uint32_t* __restrict__ tab_start,
                                                                  uint64_t* __restrict__ tab_size) {
    __shared__ fl_inflate_ws16 ws_mem;
    __shared__ uint32_t inring_mem[FL_INF_INRING / 4];
    FL_LDS fl_inflate_ws16* ws = (FL_LDS fl_inflate_ws16*)&ws_mem;
    const uint32_t lane = threadIdx.x, s = blockIdx.x;
    const uint64_t a = in_off[s];
    const uint32_t len = (uint32_t)(in_off[s + 1] - a);
    const uint64_t base = tab_off[s], cap = tab_off[s + 1] - base;
    uint32_t at = 0;
    uint64_t m = 0;
    while (m < cap) {
        fl_bitr r;
        r.data = in + a + at;
        r.nbytes = len - at;
        r.lane = lane;
        r.inring = (FL_LDS uint32_t*)inring_mem;
        const uint64_t total_bits = (uint64_t)r.nbytes * 8;
        r.left = (int64_t)total_bits;
        fl_br_seek(r, 0u);
        fl_sz_count<false> cnt;
        cnt.n = 0;
        cnt.need = 0;
        uint32_t final_seen = 0;
        uint64_t end_bit = 0;
        const int rc = fl_sz_member<false>(r, ws, container, flags, lane, true, ~0ull, total_bits, cnt, final_seen, end_bit);
        if (lane == 0) {
            tab_start[base + m] = at;
            tab_size[base + m] = rc ? 0 : cnt.n;
        }
        m++;
        if (rc) break;
        const uint32_t used = fl_uni((uint32_t)fl_br_consumed(r));
        if (!used || used >= len - at) break;  // (an accepted member is never empty)
        at += used;
    }
    if (lane == 0) tab_n[s] = m;
}

// the streams' tables back to back: dense_off = exclusive scan of tab_n (k_scan_lens)
__global__ __launch_bounds__(64) void k_member_pack(const uint64_t* __restrict__ tab_off, const uint64_t* __restrict__ tab_n,
                                                    const uint32_t* __restrict__ tab_start, const uint64_t* __restrict__ tab_size,
                                                    const uint64_t* __restrict__ dense_off, uint32_t* __restrict__ d_start,
                                                    uint64_t* __restrict__ d_size) {
    const uint32_t s = blockIdx.x;
    const uint64_t from = tab_off[s], to = dense_off[s], n = tab_n[s];
    for (uint64_t k = threadIdx.x; k < n; k += 64) {
        d_start[to + k] = tab_start[from + k];
        d_size[to + k] = tab_size[from + k];
    }
}

// One wave per stream: its members are [dense_off[s], dense_off[s + 1]).  The stream's status is the first member status
// that is not 0, in member order; out_len, consumed and n_members sum the members in front of that one.
__global__ __launch_bounds__(64) void k_member_fold(const uint64_t* __restrict__ dense_off, const uint64_t* __restrict__ m_outlen,
                                                    const int32_t* __restrict__ m_status, const uint64_t* __restrict__ m_consumed,
                                                    uint64_t* __restrict__ out_len, int32_t* __restrict__ status,
                                                    uint64_t* __restrict__ consumed, uint32_t* __restrict__ n_members) {
    const uint32_t lane = threadIdx.x, s = blockIdx.x;
    const uint64_t m0 = dense_off[s], m1 = dense_off[s + 1];
    uint64_t bad = m1;
    for (uint64_t j = m0 + lane; j < m1; j += 64)
        if (m_status[j] != 0) {
            bad = j;
            break;
        }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = __shfl_xor(bad, d, 64);
        bad = o < bad ? o : bad;
    }
    uint64_t produced = 0, used = 0;
    for (uint64_t j = m0 + lane; j < bad; j += 64) {
        produced += m_outlen[j];
        used += m_consumed[j];
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        produced += __shfl_xor(produced, d, 64);
        used += __shfl_xor(used, d, 64);
    }
    if (lane == 0) {
        out_len[s] = produced;
        status[s] = bad < m1 ? m_status[bad] : 0;
        if (consumed) consumed[s] = used;
        if (n_members) n_members[s] = (uint32_t)(bad - m0);
    }
}
