// pass_plan.h -- how compress_impl cuts a batch on the chunk path (levels 4..9, every input <= 65535 bytes; the simple
// modes) into passes, and what the two-stream path's workspace holds per pass.  Plain C++ (no HIP): flate_hip.hip uses
// it, and tests/cpu_shim compiles it for the CPU tests.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "flate_common.h"
#include "flate_layout.h"

struct fl_pass_cfg {
    uint64_t n_chunks = 0;
    uint64_t host_pass_chunks = 1024;   // FLATE_HIP_HOST_PASS_CHUNKS
    uint64_t max_pass_chunks = 32768;   // FLATE_HIP_MAX_PASS_CHUNKS
    bool pinned = false;  // a host-buffer call with pinned input or output (pinned mirrors included): sub-batches
    bool ramp = true;     // !FLATE_HIP_NO_RAMP
    bool planned = false; // flate_hip_plan_compress (device memory: never pinned)
};

struct fl_pass {
    uint64_t c0 = 0, nc = 0;
    uint32_t stream = 0;  // two-stream path: 0 = the caller's stream, 1 = the second compute stream
};

// the pass size of a call: pinned host-buffer calls run in sub-batches of host_pass_chunks (never above max_pass_chunks)
inline uint64_t fl_pass_limit(const fl_pass_cfg& c) {
    return c.pinned && !c.planned ? std::min(c.max_pass_chunks, c.host_pass_chunks) : c.max_pass_chunks;
}

// At most how many chunks the pass_index-th pass, which starts at chunk c0, takes.
// - tail merge: a sub-batch of the pinned path costs about 0.9 ms whatever it holds, so once fewer than 1.5 x the limit
//   are left the last pass takes all of them (up to max_pass_chunks): at the default 1024 it can hold 1535;
// - ramp: the GPU idles until the first sub-batch has crossed the link, so with at least 3 x the limit the first two
//   passes are a quarter and a half of it (64 at least, never above the limit).
inline uint64_t fl_pass_cap(const fl_pass_cfg& c, uint64_t c0, uint64_t pass_index) {
    const bool pinned = c.pinned && !c.planned;
    const uint64_t L = fl_pass_limit(c);
    uint64_t limit = L;
    if (pinned && c.n_chunks - c0 < L + L / 2) limit = std::min(c.max_pass_chunks, c.n_chunks - c0);
    if (c.ramp && pinned && c.n_chunks >= 3 * L && pass_index < 2)
        limit = std::min(L, std::max<uint64_t>(64, L >> (2 - pass_index)));
    return limit;
}

// The passes of a batch whose chunks all take the chunk path, in order, covering [0, n_chunks); pass k runs on stream
// k & 1 of the two-stream path, so passes k and k + 2 share a stream and a workspace slice.  Returns the largest pass.
inline uint64_t fl_pass_schedule(const fl_pass_cfg& c, std::vector<fl_pass>& out) {
    out.clear();
    uint64_t largest = 0;
    for (uint64_t c0 = 0; c0 < c.n_chunks;) {
        fl_pass p;
        p.c0 = c0;
        p.nc = std::min(fl_pass_cap(c, c0, out.size()), c.n_chunks - c0);
        p.stream = (uint32_t)(out.size() & 1u);
        out.push_back(p);
        largest = std::max(largest, p.nc);
        c0 += p.nc;
    }
    return largest;
}

// Device bytes per chunk of each buffer of a chunk-path pass's LZ workspace (ensure_lz_workspace, the two-stream slices):
// 64 KiB of positions a chunk -- the chain links (levels 4..7: kernels_parse.h) or the four link arrays [L4 | L6 | L8 | RK]
// (levels 8..9: kernels_walk.h), the anchor descriptors, the true anchors (a bit each), the tokens -- and the chunk's token
// count and flags.
struct fl_lz_sizes {
    uint64_t links, desc, marks, tokens, ntok, cflag;
};
inline fl_lz_sizes fl_lz_chunk_sizes(bool bulk_links) {
    const uint64_t per = FL_CHUNK_STRIDE;
    fl_lz_sizes z;
    z.links = bulk_links ? per * 4 * sizeof(uint16_t) : per * sizeof(uint16_t);
    z.desc = per * sizeof(uint32_t);
    z.marks = per / 8;
    z.tokens = per * sizeof(uint32_t);
    z.ntok = sizeof(uint32_t);
    z.cflag = sizeof(uint32_t);
    return z;
}
inline uint64_t fl_lz_chunk_bytes(bool bulk_links) {
    const fl_lz_sizes z = fl_lz_chunk_sizes(bulk_links);
    return z.links + z.desc + z.marks + z.tokens + z.ntok + z.cflag;
}

// ... and per block slot: its plan, its histograms, its two checksum words
struct fl_blk_sizes {
    uint64_t plan, hist, cks;
};
inline fl_blk_sizes fl_block_slot_sizes() {
    fl_blk_sizes b;
    b.plan = sizeof(fl_block_plan);
    b.hist = 320 * sizeof(uint32_t);
    b.cks = 2 * sizeof(uint32_t);
    return b;
}
inline uint64_t fl_block_bytes() {
    const fl_blk_sizes b = fl_block_slot_sizes();
    return b.plan + b.hist + b.cks;
}
