// inflate_plan.h -- host side of the inflate entry points (flate_hip.hip: decompress_core, flate_hip_decompress_batch_dict,
// flate_hip_decompressed_sizes, flate_hip_decompress_members, flate_hip_decompress_ranges, index_walk): the chunk table
// they hand the kernels, which LDS ring a launch gets, when a host call with pinned buffers runs in sub-batches and how
// large those are, when k_inflate_par runs before k_inflate, when the span pool is given back, and how a host caller's
// output comes home -- and of the resumable inflater's host feeds (flate_hip_inflater_feed): which slots it takes, the
// offsets it stages, how the produced bytes come home.  Plain C++ (no HIP types): flate_hip.hip uses it, tests/cpu_shim
// compiles it for the CPU tests.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "flate_layout.h"

// ---- the chunk table

#define FL_INF_MAX_IN_BYTES 0xfffffff0ull  // compressed bytes of one stream, at most (fl_chunk::in_len is 32 bits)

// The first stream of hin[0..n] (ascending) that is longer than FL_INF_MAX_IN_BYTES; n: none is.
inline uint32_t fl_inflate_oversize(const uint64_t* hin, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (hin[i + 1] - hin[i] > FL_INF_MAX_IN_BYTES) return i;
    return n;
}

// The table of a call over streams hin[0..n] whose slots are hout[0..n] (nullptr: the call writes no output -- the size
// probe, the index walk); in_shift / out_shift: what the device's offsets are less than the caller's (a host caller's
// buffers are staged from their first byte).  Everything else of an entry is 0; a caller that skips streams sets
// fl_chunk::skip itself.  False, and the table is not to be used: a stream is longer than FL_INF_MAX_IN_BYTES.
inline bool fl_inflate_chunks(const uint64_t* hin, const uint64_t* hout, uint32_t n, uint64_t in_shift, uint64_t out_shift,
                              std::vector<fl_chunk>& chunks) {
    chunks.assign(n, fl_chunk{});
    if (fl_inflate_oversize(hin, n) != n) return false;
    for (uint32_t i = 0; i < n; i++) {
        fl_chunk& c = chunks[i];
        c.in_off = hin[i] - in_shift;
        c.in_len = (uint32_t)(hin[i + 1] - hin[i]);
        if (hout) {
            c.out_off = hout[i] - out_shift;
            c.out_cap = hout[i + 1] - hout[i];
        }
    }
    return true;
}

// ---- the LDS ring of k_inflate, k_inflate_dict and k_inflate_range (a wave per stream)

#define FL_INF_RING_LARGE_STREAMS (4u * 256u)  // launches of up to this many streams get the large ring (measured crossover)

// few streams: the latency of one stream decides, give each the large LDS ring (3 per CU);
// many streams: the small ring keeps 20 per CU in flight
// knob: FLATE_HIP_INFLATE_RING (-1 unset; else the ring's size in bytes, the large ring from FL_INF_RING_LARGE on)
inline bool fl_inflate_ring_large(int64_t knob, uint32_t n_streams) {
    return knob >= 0 ? knob >= (int64_t)FL_INF_RING_LARGE : n_streams <= FL_INF_RING_LARGE_STREAMS;
}

// ---- host calls with pinned buffers: sub-batches with the copies on their own streams

#define FL_INF_PIN_OUT_PER_IN 8ull           // the slots may be this many times the input ...
#define FL_INF_PIN_OUT_SLACK (1ull << 20)    // ... and this many bytes more
#define FL_INF_PIN_MIN_PASSES 4u             // more streams than this many times FLATE_HIP_HOST_PASS_CHUNKS
#define FL_INF_PIN_SUB_PASSES 3u             // a sub-batch: this many times FLATE_HIP_HOST_PASS_CHUNKS streams, about

// Pinned host buffers whose output slots are not much larger than what goes in (a caller who knows
// the sizes): sub-batches with the copies on their own streams, as in compress_impl.  Otherwise one
// staged copy in, and only the produced bytes come back (copy_out_host).
inline bool fl_inflate_pin_io(bool in_pinned, bool out_pinned, uint64_t in_bytes, uint64_t out_bytes, uint32_t n_streams,
                              size_t host_pass_chunks) {
    return in_pinned && out_pinned && out_bytes <= FL_INF_PIN_OUT_PER_IN * in_bytes + FL_INF_PIN_OUT_SLACK &&
           n_streams > FL_INF_PIN_MIN_PASSES * host_pass_chunks;
}

// Streams per sub-batch of such a call (the last one has what is left).
// (a wave per stream: a sub-batch must still fill the chip -- 20 streams per CU -- or the kernel's latency per
// stream, not the copies, decides; measured: sub-batches of 1024 streams are slower than no overlap at all: two sub-batches
// of 2049 streams take as long as one batch, five of 3277 are 33 GB/s against 24, tools/e2e_inflate_probe.py)
// sub-batches of one size (4097 streams used to be 4096 + 1, and the launch for the one cost a stream's whole latency)
// (Two guards that the rule did not have while it stood in decompress_core, neither reachable with a knob the library
// accepts and a batch that fits a device: the sum is rounded up in 64 bits -- with n_streams + nsub beyond 2^32 it came to 0
// streams a sub-batch, a loop that does not end -- and a target of 0, a knob that is a multiple of 2^32, counts as 1.)
inline uint32_t fl_inflate_sub_batch(uint32_t n_streams, size_t host_pass_chunks) {
    const uint32_t target = FL_INF_PIN_SUB_PASSES * (uint32_t)host_pass_chunks;
    const uint32_t nsub = std::max(1u, n_streams / std::max(target, 1u));
    return (uint32_t)(((uint64_t)n_streams + nsub - 1) / nsub);
}

// ---- k_inflate_par before k_inflate

#define FL_INF_PAR_MIN_BYTES 32768u   // FLATE_HIP_INFLATE_PAR unset: a stream of this many compressed bytes is long
#define FL_INF_PAR_SLOT_PER_IN 16ull  // ... and so is one whose output slot is this many times that
#define FL_INF_PAR_MAX_BIG 2048u      // long streams of a call beyond which every stream is k_inflate's

struct fl_inflate_par {
    bool use = false;        // k_inflate_par runs over every launch of the call
    uint32_t min_bytes = 0;  // what it is told a long stream is
    uint32_t n_big = 0;
    uint64_t taken = 0;      // streams it is launched for (flate_hip_debug_inflate_paths): those the spans left
};

// Long streams of a batch that has few of them: a workgroup per stream (kernels_inflate_par.h).  It marks
// what it does not finish (short streams, anything irregular) FL_PAR_REDO, and k_inflate takes those.
// knob: FLATE_HIP_INFLATE_PAR -- -1: unset; 0: never; else the minimum stream size in bytes.  Never with the strict
// header of flags & 1.
inline fl_inflate_par fl_inflate_par_plan(const fl_chunk* chunks, uint32_t n, int64_t knob, int flags) {
    fl_inflate_par p;
    p.min_bytes = knob >= 0 ? (uint32_t)knob : FL_INF_PAR_MIN_BYTES;
    for (uint32_t i = 0; i < n; i++)  // long input, or an output slot that says the output is long
        p.n_big += (chunks[i].in_len >= p.min_bytes || chunks[i].out_cap >= FL_INF_PAR_SLOT_PER_IN * p.min_bytes) ? 1u : 0u;
    p.use = p.min_bytes && p.n_big && p.n_big <= FL_INF_PAR_MAX_BIG && !(flags & 1);
    for (uint32_t i = 0; p.use && i < n; i++) p.taken += chunks[i].skip ? 0u : 1u;
    return p;
}

// ---- the span pool

#define FL_INF_POOL_KEEP_BYTES (2ull << 30)

// (the pool holds a second copy of the decoded output: a large one does not stay with the handle)
inline bool fl_inflate_pool_release(uint64_t pool_bytes) { return pool_bytes > FL_INF_POOL_KEEP_BYTES; }

// ---- a host caller's output on its way home (copy_out_host)

enum fl_copy_out_kind { FL_COPY_OUT_NONE = 0, FL_COPY_OUT_DENSE = 1, FL_COPY_OUT_PACKED = 2 };
struct fl_copy_out {
    int kind = FL_COPY_OUT_NONE;
    uint64_t total = 0;  // bytes produced
    uint64_t end = 0;    // dense: the end of the last produced byte (an offset of the caller's)
};

// The slots are sized for the worst case (an inflate caller may reserve 1000x the input): when the produced bytes are
// less than half of the slot range hout[0]..hout[n] they come home packed, otherwise the range from the first slot to
// the end of the last produced byte is copied as it is.  Nothing produced, or no slots: nothing to copy.
inline fl_copy_out fl_copy_out_plan(const uint64_t* hout, const uint64_t* out_len, uint32_t n) {
    fl_copy_out p;
    const uint64_t out_lo = hout[0], out_hi = hout[n];
    if (out_hi <= out_lo) return p;
    for (uint32_t i = 0; i < n; i++) p.total += out_len[i];
    if (p.total == 0) return p;
    if (p.total * 2 < out_hi - out_lo) {
        p.kind = FL_COPY_OUT_PACKED;
        return p;
    }
    p.kind = FL_COPY_OUT_DENSE;
    p.end = out_lo;
    for (uint32_t i = 0; i < n; i++)
        if (out_len[i]) p.end = std::max(p.end, hout[i] + out_len[i]);
    return p;
}

// ---- the resumable inflater's host feeds (flate_hip_inflater_feed with FLATE_HIP_MEM_HOST)

#define FL_INFLATER_MIN_SLOT 258u      // a slot is empty or at least the longest match: such a feed always makes progress
#define FL_INFLATER_COPY_EACH_MAX 16u  // up to this many streams, each stream's bytes come home by a copy of their own

// The caller's tables (n + 1 offsets each, n final flags): the offsets ascend, and the slot of a stream that is not
// skipped -- an empty piece, final 0 and an empty slot -- is empty or at least FL_INFLATER_MIN_SLOT bytes.
inline bool fl_inflater_slots_ok(const uint64_t* in_off, const uint64_t* out_off, const uint8_t* final_, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        if (in_off[i + 1] < in_off[i] || out_off[i + 1] < out_off[i]) return false;
        const uint64_t slot = out_off[i + 1] - out_off[i];
        const bool skipped = in_off[i + 1] == in_off[i] && !final_[i] && slot == 0;
        if (!skipped && slot > 0 && slot < FL_INFLATER_MIN_SLOT) return false;
    }
    return true;
}

// The pieces and the slots are staged from their first byte: the offsets the kernel sees start at 0
inline void fl_inflater_rebase(const uint64_t* in_off, const uint64_t* out_off, uint32_t n, std::vector<uint64_t>& hin,
                               std::vector<uint64_t>& hout) {
    hin.resize((size_t)n + 1);
    hout.resize((size_t)n + 1);
    for (uint32_t i = 0; i <= n; i++) {
        hin[i] = in_off[i] - in_off[0];
        hout[i] = out_off[i] - out_off[0];
    }
}

// Only the produced bytes reach the caller's slots (what lies beyond out_len[i] stays as it was): a few streams by a
// copy each from the device, many by one copy of all slots to the host and a memcpy of each stream's bytes from there.
inline bool fl_inflater_copy_each(uint32_t n) { return n <= FL_INFLATER_COPY_EACH_MAX; }
