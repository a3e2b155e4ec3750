// pass_plan.h -- the host decisions of compress_impl (flate_hip.hip), which only carries them out: the chunk table of a
// batch (fl_chunk_table), how the batch is cut into passes -- runs of consecutive chunks of one kind, chunk path or
// whole-stream path (fl_pass_next; fl_pass_schedule is its all-chunk case) --, the block tables of a pass
// (fl_pass_tables, fl_chunk_blocks), when the passes alternate between two compute streams and what each stream's
// workspace slice holds (fl_two_eligible, fl_two_from_plan, fl_two_from_schedule, the bytes per chunk and per block),
// and which rows of a pass's output slots go home by a rectangle copy (fl_rect_rows).  Plain C++ (no HIP): flate_hip.hip
// uses it, tests/cpu_shim compiles it for the CPU tests and tests/host_cpp/test_pass_plan.cpp walks it under sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/flate_hip.h"
#include "flate_common.h"
#include "flate_layout.h"
#include "stream_tables.h"

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

// The chunk table of a batch: where every input lies and how much room its output slot has, with the staging shifts
// taken off (host buffers are staged from their first byte on).  false: an input is too long.
inline bool fl_chunk_table(const uint64_t* hin, const uint64_t* hout, uint32_t n_chunks, uint64_t in_shift, uint64_t out_shift,
                           int mode, const FlushSpec* fs, std::vector<fl_chunk>& chunks) {
    chunks.assign(n_chunks, fl_chunk{});
    for (uint32_t i = 0; i < n_chunks; i++) {
        fl_chunk& c = chunks[i];
        const uint64_t len = hin[i + 1] - hin[i];
        c.in_off = hin[i] - in_shift;
        c.out_off = hout[i] - out_shift;
        c.out_cap = hout[i + 1] - hout[i];
        c.skip = 0;
        // stream positions are 32-bit and the last match tile looks 64 KiB + 258 bytes ahead of its start
        if (len > (mode >= 4 ? 0xfff00000ull : 0xfffffff0ull)) return false;
        c.in_len = (uint32_t)len;
        c.pos_off = 0;
        c.piece0 = c.n_piece = c.flush_off = c.n_flush = c.zone_off = c.n_slides = 0;
        c.unfinished = (fs && !fs->finish) ? 1u : 0u;
        c.pad_ = 0;
    }
    return true;
}

// A pass is a run of consecutive chunks of one kind: at levels 4..9 inputs of up to 65535 bytes
// take the chunk path (kernels_lz.h), longer ones -- and every stream with flush points -- the whole-stream path
// (kernels_stream.h).
inline bool fl_whole_stream(int mode, bool has_flush, uint32_t in_len) {
    return mode >= 4 && (has_flush || in_len > FLATE_HIP_MAX_LZ_CHUNK);
}

struct fl_pass_pick {
    uint32_t nc = 0;      // chunks of the pass (never 0 while chunks are left)
    bool stream = false;  // a whole-stream pass
};

// The pass_index-th pass of a batch, which starts at chunk c0: a chunk pass ends at fl_pass_cap, a whole-stream pass
// before the stream that would take it past stream_pass_bytes uncompressed bytes (about 30 bytes of scratch per input
// byte) -- its first stream is always taken --, and either at the first chunk of the other kind.  pass_index counts the
// passes of both kinds.  chunks == nullptr: every chunk takes the chunk path (fl_pass_schedule).
inline fl_pass_pick fl_pass_next(const fl_pass_cfg& cfg, const fl_chunk* chunks, uint64_t c0, uint64_t pass_index, int mode,
                                 bool has_flush, uint64_t stream_pass_bytes) {
    fl_pass_pick pk;
    pk.stream = chunks && fl_whole_stream(mode, has_flush, chunks[c0].in_len);
    uint64_t pass_bytes = 0, nc = 0;
    // (a sub-batch of the pinned path costs about 0.9 ms whatever it holds: a tail of less than half a sub-batch
    // goes with the one before it)
    // (the GPU idles until the first sub-batch has crossed the link: the first two are a quarter and a half)
    const uint64_t limit = fl_pass_cap(cfg, c0, pass_index);
    if (!chunks) nc = std::min(limit, cfg.n_chunks - c0);
    for (; chunks && c0 + nc < cfg.n_chunks; nc++) {
        const fl_chunk& c = chunks[c0 + nc];
        if (fl_whole_stream(mode, has_flush, c.in_len) != pk.stream) break;
        if (pk.stream ? (nc > 0 && pass_bytes + c.in_len > stream_pass_bytes) : nc >= limit) break;
        pass_bytes += c.in_len;
    }
    pk.nc = (uint32_t)nc;
    return pk;
}

// The passes of a batch whose chunks all take the chunk path, in order, covering [0, n_chunks); pass k runs on stream
// k & 1 of the two-stream path, so passes k and k + 2 share a stream and a workspace slice.  Returns the largest pass.
inline uint64_t fl_pass_schedule(const fl_pass_cfg& c, std::vector<fl_pass>& out) {
    out.clear();
    uint64_t largest = 0;
    for (uint64_t c0 = 0; c0 < c.n_chunks;) {
        fl_pass p;
        p.c0 = c0;
        p.nc = fl_pass_next(c, nullptr, c0, out.size(), 0, false, 0).nc;
        p.stream = (uint32_t)(out.size() & 1u);
        out.push_back(p);
        largest = std::max(largest, p.nc);
        c0 += p.nc;
    }
    return largest;
}

// Block slots of a chunk on the chunk path: two at levels 4..9, and in the simple modes a block per full 65535-byte
// buffer and one for what is left, an empty one if nothing (deflate.zig:498-511, 480-484).
inline uint32_t fl_chunk_blocks(int mode, uint32_t in_len) { return mode >= 4 ? 2u : in_len / FL_BLOCK_BYTES + 1; }

// Block slots of all chunk passes of a batch without flush points (the pinned path lays out a slice of the block -> chunk
// table per pass before the first one): the sum of what fl_pass_tables returns for them.
inline uint64_t fl_batch_blocks(const fl_chunk* chunks, uint32_t n_chunks, int mode) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_chunks; i++) total += fl_chunk_blocks(mode, chunks[i].in_len);
    return total;
}

// The block tables of the pass chunks[0 .. nc): first_block, n_blocks and pos_off of every chunk, the pass's block ->
// chunk table, and for a whole-stream pass its StreamTables, for a simple mode with flush points its fl_sblock list
// (huffman-only / store-only).  Returns the pass's number of blocks (= blk_chunk.size()).
inline uint32_t fl_pass_tables(fl_chunk* chunks, uint32_t nc, bool stream, int mode, const FlushSpec* fs, StreamTables& tabs,
                               std::vector<uint32_t>& blk_chunk, std::vector<fl_sblock>& sblocks) {
    uint32_t nb = 0;
    for (uint32_t i = 0; i < nc; i++) {
        fl_chunk& c = chunks[i];
        c.first_block = nb;
        if (stream) {
            add_stream_chunk(tabs, c, i, nb, fs);
        } else if (fs) {
            // SimpleCompressor (deflate.zig:449-529): the 65535-byte buffer goes out as soon as it is
            // full; flush / finish write what it holds then, an empty block if nothing (474-484)
            uint32_t prev = 0;
            auto piece = [&](uint32_t start, uint32_t end, bool last) {
                uint32_t p = start;
                for (; end - p >= FL_BLOCK_BYTES; p += FL_BLOCK_BYTES) sblocks.push_back(fl_sblock{p, FL_BLOCK_BYTES, 0u});
                sblocks.push_back(fl_sblock{p, end - p, last ? 1u : 0u});
                if (!last) sblocks.push_back(fl_sblock{0u, 0u, 2u});
            };
            for (uint32_t k = 0; k < fs->n; k++) {
                piece(prev, (uint32_t)fs->pos[k], false);
                prev = (uint32_t)fs->pos[k];
            }
            if (fs->finish) piece(prev, c.in_len, true);
            c.n_blocks = (uint32_t)sblocks.size();
            c.pos_off = 0;
        } else {
            c.n_blocks = fl_chunk_blocks(mode, c.in_len);
            c.pos_off = (uint64_t)i * FL_CHUNK_STRIDE;
        }
        for (uint32_t k = 0; k < c.n_blocks; k++) blk_chunk.push_back(i);
        nb += c.n_blocks;
    }
    return nb;
}

// Round 6: TWO compute streams.  A sub-batch's six kernels each end in a tail that fills the chip less and less (1024 chunks are
// four per CU: 2.15 ms a sub-batch where a quarter of the whole batch's 6.6 ms would be 1.65) and the next sub-batch's first
// kernel waits behind the last one's tail.  The sub-batches alternate between the caller's stream and a second one -- every
// per-pass buffer has a slice per stream, so two passes that may run at once never touch the same bytes -- and the kernels of sub-batch
// k + 1 start as soon as its input is there and run into the tails of k's: 10.3 -> 10.0 ms per 256 MiB in one process, 11.7 ->
// 10.1 in another (bench e2e_host).  Levels 4-9, every input on the chunk path.  What lost (profiles/r06_host_path.txt): the
// tokenizers of all sub-batches in a row on one stream with the chains and the back ends on streams of higher priority beside
// them, 11.0 ms -- k_lz_parse takes a CU's whole LDS, a single small workgroup on a CU keeps the next tokenizer workgroup off it,
// and every kernel ran a quarter to a half longer than alone.
// (planned device batches of more than one pass take the same way: flate_hip_compress_planned)
// pinned_passes: a host-buffer call with pinned input or output that is not planned; planned_passes: the passes of the
// plan a planned call runs (0: not such a call).
inline bool fl_two_eligible(const fl_pass_cfg& cfg, bool pinned_passes, size_t planned_passes, int mode, bool has_flush,
                            bool one_stream, const fl_chunk* chunks) {
    bool two = ((pinned_passes && cfg.n_chunks > fl_pass_limit(cfg)) || planned_passes > 1) && mode >= 4 && !has_flush && !one_stream;
    for (uint64_t i = 0; two && i < cfg.n_chunks; i++) two = chunks[i].in_len <= FLATE_HIP_MAX_LZ_CHUNK;
    return two;
}

// The two streams' workspace is TWO slices of every per-pass buffer, each as large as the largest pass (the
// merged tail, not the sub-batch size); pass k runs on stream k & 1 in slice k & 1.  Passes k and k + 2 run in order on one
// stream, so pass k + 2 reuses pass k's bytes only after pass k's last kernel.
struct fl_two_slices {
    std::vector<fl_pass> sched;  // the passes of the two-stream path
    uint64_t nc = 0, nb = 0;     // chunks and block slots of one slice
};
// ... of a plan's passes (anything with .nc and .nb).  false: fewer than two passes, a second slice would never be used.
template <class Passes>
inline bool fl_two_from_plan(const Passes& passes, fl_two_slices& s) {
    s = fl_two_slices();
    for (size_t k = 0; k < passes.size(); k++) {
        fl_pass p;
        p.c0 = s.sched.empty() ? 0 : s.sched.back().c0 + s.sched.back().nc;
        p.nc = passes[k].nc;
        p.stream = (uint32_t)(k & 1u);
        s.sched.push_back(p);
        s.nc = std::max<uint64_t>(s.nc, passes[k].nc);
        s.nb = std::max<uint64_t>(s.nb, passes[k].nb);
    }
    return s.sched.size() >= 2;
}
// ... of a batch that is cut here
inline bool fl_two_from_schedule(const fl_pass_cfg& cfg, fl_two_slices& s) {
    s = fl_two_slices();
    s.nc = fl_pass_schedule(cfg, s.sched);
    s.nb = 2 * s.nc;  // (levels 4..9 on the chunk path: two block slots per chunk)
    // (up to 1.5 x the limit the merged tail is ONE pass: a second slice would never be used)
    return s.sched.size() >= 2;
}

// Slots of one size (the usual case: compress_bound of one chunk size): the first half of every slot goes
// home by the DMA engine's rectangle copy -- what lies beyond out_len[i] there is the zeros the slots were
// cleared with --, and only what a chunk produced BEYOND that half by the copy kernel: a few workgroups that
// take the slots in turn.  The kernel is not free beside the next sub-batch's kernels: its stores wait for the
// link and the stores of the other kernels wait behind them (k_lz_chain took 0.47 ms instead of 0.09 beside
// it, started behind it the tokenizer paid the same); the DMA engine costs them nothing (11.7 -> 10.5 ms for
// 256 MiB of text, where no chunk reaches the second half).
struct fl_rect {
    uint32_t urows = 0;            // the pass's first slots, all of one size, that take the rectangle copy (0: none)
    uint64_t pitch = 0, half = 0;  // their size, and how much of each the rectangle holds
};
// slot: the nc + 1 offsets of the pass's output slots; rect_knob: FLATE_HIP_RECT (-1 unset)
inline fl_rect fl_rect_rows(const uint64_t* slot, uint32_t nc, int rect_knob) {
    fl_rect r;
    if (nc > 1) {
        r.pitch = slot[1] - slot[0];
        for (r.urows = 1; r.urows < nc && slot[r.urows + 1] - slot[r.urows] == r.pitch; r.urows++) {}
        r.half = (r.pitch / 2) & ~(uint64_t)15;
        // (Round 5: OFF unless FLATE_HIP_RECT=1.  The rectangle copy is a DMA copy that waits for the sub-batch's kernels
        // -- and the input copy of the NEXT sub-batch, submitted behind it, lands in the same in-order DMA queue in most
        // calls of a process: then nothing overlaps any more, 16.6 ms per 256 MiB instead of 10.4 (rocprofv3 timelines,
        // profiles/r05_host_path.txt: the 10.4 only ever showed in the second call of a process).  The copy kernel
        // alone is 11.4 ms in every call.)
        if (r.urows < 64 || r.half < 4096 || rect_knob != 1) r.urows = 0;
    }
    return r;
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
