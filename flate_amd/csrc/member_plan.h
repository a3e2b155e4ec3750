// member_plan.h -- the rules of flate_hip_decompress_members that are the same text on the device and on the CPU: how a
// probed member start ("candidate") finds the candidate behind it, what a walk that lands on a byte no member can start at
// reports, how the chain of a stream's members is followed through its successor table (from a tile of it at a time), and
// how the host lays the members' output slots out.  Plain C++ (no HIP types): kernels_members.h and flate_hip.hip use it,
// tests/cpu_shim compiles it for the CPU tests.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FL_MP_HD __host__ __device__ inline
#else
#define FL_MP_HD inline
#endif

#define FL_MEM_SCAN_TILE 16384u  // bytes of the input a wave of k_member_scan searches (16 bytes a lane and step)
#define FL_MEM_LDS_TILE 2048u    // successors of a stream that k_member_chain holds in LDS at a time
#define FL_MEM_CAND_DEFAULT (1u << 22)  // FLATE_HIP_MEMBER_CANDIDATES: candidates of a call beyond which it walks instead

// what a successor entry says when it is no index
#define FL_MEM_END 0xffffffffu   // the member ends where the stream ends: the chain is complete
#define FL_MEM_MISS 0xfffffffeu  // the member ends at a byte that is no candidate: a failing remainder starts there
#define FL_MEM_ERR 0xfffffffdu   // the probe refused this candidate: it is the failing remainder itself

// the least a member of a container can take of the input when it is accepted (header, an empty fixed block, footer):
// what bounds the members of a stream of n bytes by n / least + 1 (the one more fails)
FL_MP_HD uint32_t fl_member_least_bytes(int container) { return container == 1 ? 20u : container == 2 ? 8u : 2u; }

// first index in pos[0..n) (ascending) that is not below key
FL_MP_HD uint32_t fl_member_lower_bound(const uint64_t* pos, uint32_t n, uint64_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pos[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// last stream i of off[0..n] (ascending, n >= 1) with off[i] <= p; p >= off[0]
FL_MP_HD uint32_t fl_member_stream_of(const uint64_t* off, uint32_t n, uint64_t p) {
    uint32_t lo = 0, hi = n;  // off[lo] <= p, and off[hi] > p or hi == n
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// The successor of candidate i of a stream whose candidates are pos[0..n) (ascending, absolute) and that ends at
// stream_end: the candidate at which the next member starts, or one of the three words above.
FL_MP_HD uint32_t fl_member_successor(const uint64_t* pos, uint32_t n, uint32_t i, int32_t status, uint64_t consumed,
                                      uint64_t stream_end) {
    if (status != 0) return FL_MEM_ERR;
    const uint64_t next = pos[i] + consumed;
    if (next >= stream_end) return FL_MEM_END;  // (never beyond it: the probe was given the stream's bytes alone)
    const uint32_t j = fl_member_lower_bound(pos, n, next);
    return j < n && pos[j] == next ? j : FL_MEM_MISS;
}

// What decoding a gzip member reports at a position that does not read 1f 8b 08 (or has no room to): fl_inf_header reads
// the 10 fixed bytes before it compares any, so fewer than 10 are EndOfStream (1) and anything else BadGzipHeader (2).
FL_MP_HD int32_t fl_member_miss_status(uint64_t bytes_left) { return bytes_left < 10 ? 1 : 2; }

// Follow a stream's chain.  succ[0..n): the successors of its candidates; first: the candidate at the stream's first
// byte, or FL_MEM_MISS when there is none.  tile[0..FL_MEM_LDS_TILE) is scratch (LDS on the device) that lanes
// lane, lane + nlanes, ... fill together, sync() between its writers and readers; every lane walks the same chain.
// Lane 0 writes the candidates on the chain to chain[0..) -- at most n, a successor is always behind its candidate --
// and the walk's last word (FL_MEM_END / MISS / ERR) to *stop.  Returns how many candidates are on the chain.
template <class Sync, class Uni>
FL_MP_HD uint32_t fl_member_follow(const uint32_t* succ, uint32_t n, uint32_t first, uint32_t* tile, uint32_t lane,
                                   uint32_t nlanes, Sync sync, Uni uni, uint32_t* chain, uint32_t* stop) {
    uint32_t cur = first, count = 0, t0 = 0, have = 0;  // tile holds succ[t0 .. t0 + have)
    while (cur < n && count < n) {
        if (cur - t0 >= have) {  // (unsigned: also cur < t0, which never happens)
            sync();
            t0 = cur;
            have = n - t0 < FL_MEM_LDS_TILE ? n - t0 : FL_MEM_LDS_TILE;
            for (uint32_t k = lane; k < have; k += nlanes) tile[k] = succ[t0 + k];
            sync();
        }
        if (lane == 0) chain[count] = cur;
        count++;
        const uint32_t next = uni(tile[cur - t0]);
        cur = next < n && next <= cur ? FL_MEM_MISS : next;  // (a table that goes backwards is no chain: stop)
    }
    if (lane == 0) *stop = cur < n ? FL_MEM_MISS : cur;
    return count;
}

// The stream's table from its chain: an entry (start relative to the stream, probed size) per candidate on the chain and,
// where the walk ended at a byte that is no candidate, one more for the failing remainder that starts there.  (A candidate
// the probe refused is the chain's last entry and is that remainder itself.)  Lanes share the entries; returns their number.
FL_MP_HD uint32_t fl_member_table(const uint32_t* chain, uint32_t count, uint32_t stop, const uint64_t* pos,
                                  const uint64_t* consumed, const uint64_t* size, uint64_t stream_start, uint32_t lane,
                                  uint32_t nlanes, uint32_t* tab_start, uint64_t* tab_size) {
    for (uint32_t k = lane; k < count; k += nlanes) {
        const uint32_t c = chain[k];
        tab_start[k] = (uint32_t)(pos[c] - stream_start);
        tab_size[k] = size[c];
    }
    if (stop != FL_MEM_MISS) return count;
    if (lane == 0) {
        uint64_t at = stream_start;
        if (count) at = pos[chain[count - 1]] + consumed[chain[count - 1]];
        tab_start[count] = (uint32_t)(at - stream_start);
        tab_size[count] = 0;
    }
    return count + 1;
}

// The output slots of one stream's members: member k starts where the probed sizes of the members before it end,
// clamped to the stream's slot; the last member owns the rest.  Writes out[0..m) (starts); the caller closes the
// partition with slot_end.
FL_MP_HD void fl_member_slots(const uint64_t* size, uint32_t m, uint64_t slot_start, uint64_t slot_end, uint64_t* out) {
    uint64_t at = slot_start;
    for (uint32_t k = 0; k < m; k++) {
        out[k] = at;
        const uint64_t room = slot_end - at;
        at += size[k] < room ? size[k] : room;
    }
}

// ---- the host's side of flate_hip_decompress_members (flate_hip.hip)

#define FL_MEM_MAX_TILES 0x7fffffffull    // tiles of a scan: a workgroup each, the grid's x
#define FL_MEM_MAX_MEMBERS 0xfffffff0ull  // members of a call: they are decoded as one batch, whose count is 32 bits

// The scan's tiles over the input bytes [lo, hi) (offsets into the buffer at address `base`): a lane reads 16 bytes at an
// address that is a multiple of 16, so the first tile starts at rel0 <= lo (it may be negative: the bytes before lo are
// not looked at), up to 15 bytes before it.  False: more tiles than a grid has workgroups.
struct fl_member_tiles {
    int64_t rel0 = 0;
    uint64_t n_tiles = 0;
};
inline bool fl_member_scan_tiles(uint64_t base, uint64_t lo, uint64_t hi, fl_member_tiles& t) {
    const uint64_t first = base + lo;
    t.rel0 = (int64_t)lo - (int64_t)(first & 15);
    t.n_tiles = (uint64_t)((int64_t)hi - t.rel0 + FL_MEM_SCAN_TILE - 1) / FL_MEM_SCAN_TILE;
    return t.n_tiles <= FL_MEM_MAX_TILES;
}

// Entries of all member tables together, at most.  Scan: every candidate is on at most one chain, and a stream's table
// has at most one entry more than its chain (the failing remainder).
inline uint64_t fl_member_scan_cap(uint64_t n_cand, uint32_t n_streams) { return n_cand + n_streams; }

// Walk: a stream of len bytes has at most len / least + 1 members, and one entry more for the remainder; toff[0..n] is
// where every stream's table starts in the one array (k_member_walk's).  Returns toff[n], the capacity.
inline uint64_t fl_member_walk_offsets(const uint64_t* hin, uint32_t n, int container, uint64_t* toff) {
    const uint32_t least = fl_member_least_bytes(container);
    uint64_t cap = 0;
    for (uint32_t i = 0; i < n; i++) {
        toff[i] = cap;
        cap += (hin[i + 1] - hin[i]) / least + 2;
    }
    toff[n] = cap;
    return cap;
}

// The number of members that came back: every stream has at least one entry, and the tables hold no more than cap.
inline bool fl_member_count_ok(uint64_t M, uint32_t n_streams, uint64_t cap) {
    return !(M < n_streams || M > cap || M > FL_MEM_MAX_MEMBERS);
}

// What is wrong with the table of a stream
enum fl_member_fault { FL_MEM_TAB_OK = 0, FL_MEM_TAB_NO_FIRST = 1, FL_MEM_TAB_ORDER = 2 };
struct fl_member_verdict {
    int fault = FL_MEM_TAB_OK;
    uint32_t stream = 0;  // the first stream whose table is refused
};

// The members as a batch of their own: a contiguous partition of the input and of the slots.  doff[0..n]: where every
// stream's entries are in mstart / msize (a prefix sum of the table lengths: ascending from 0, doff[n] = M entries, which
// fl_member_count_ok has seen); vin / vout[0..n]: the streams' input offsets and slots as the kernels see them.  Writes
// min_ / mout[0..M]: the members' input offsets and slots.  A stream's table is refused when it is empty or its first
// member does not start at the stream's first byte (NO_FIRST), and when a start goes backwards or lies beyond the
// stream's end (ORDER); min_ / mout are then not to be used.
inline fl_member_verdict fl_member_partition(const uint64_t* doff, const uint32_t* mstart, const uint64_t* msize, const uint64_t* vin,
                                             const uint64_t* vout, uint32_t n, uint64_t* min_, uint64_t* mout) {
    fl_member_verdict v;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t m0 = doff[i], m = doff[i + 1] - m0;
        v.stream = i;
        if (m == 0 || mstart[m0] != 0) {
            v.fault = FL_MEM_TAB_NO_FIRST;
            return v;
        }
        for (uint64_t k = 0; k < m; k++) {
            min_[m0 + k] = vin[i] + mstart[m0 + k];
            if (min_[m0 + k] > vin[i + 1] || (k && mstart[m0 + k] < mstart[m0 + k - 1])) {
                v.fault = FL_MEM_TAB_ORDER;
                return v;
            }
        }
        fl_member_slots(msize + m0, (uint32_t)m, vout[i], vout[i + 1], mout + m0);
    }
    v.stream = 0;
    min_[doff[n]] = vin[n];
    mout[doff[n]] = vout[n];
    return v;
}
