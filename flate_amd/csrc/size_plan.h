// size_plan.h -- host side of flate_hip_decompressed_sizes for long streams: which streams of a batch are cut, where the
// scan for block starts is aimed, and whether the records of a stream's spans form a closed chain whose lengths may be
// summed.  Plain C++ (no HIP types): flate_hip.hip uses it, kernels_inflate_size.h shares the two records, and
// tests/cpu_shim compiles it for the CPU tests.
#pragma once
#include <stdint.h>

#include <vector>

#define FL_SZ_SPAN_BYTES 16384u  // compressed bytes between two scan targets, at least
#define FL_SZ_SPAN_MAX 1024u     // scan targets per call, at most (a target is a workgroup of k_span_scan)
#define FL_SZ_STREAMS_MAX 256u   // streams cut per call, at most
#define FL_SZ_LONG_BYTES 32768u  // a stream of this many bytes counts as long

// one span of a stream, as the counting kernel is given it
struct fl_size_span {
    uint64_t start_bit;  // a block starts here (0 with first: the container's header does)
    uint64_t stop_bit;   // the span ends in front of the first block that begins at or behind this position (~0: never)
    uint32_t stream;
    uint32_t first;      // the stream's first span: it parses the container's header
};
// ... and what the kernel says about it
struct fl_size_rec {
    uint64_t end_bit;    // where the block behind the span's last one begins (final_seen: where the last block ended)
    uint64_t out_len;    // bytes the span's blocks produce
    uint64_t need_hist;  // largest (distance - bytes the span had produced before the match), 0: no match leaves the span
    uint64_t consumed;   // final_seen: input bytes of the member, footer included
    int32_t status;
    uint32_t final_seen;  // the span decoded the block with BFINAL and read the footer
};

// Which streams are cut.  Cutting pays when a wave per stream would leave most of the chip idle: at most n_cu long
// streams in the batch (a CU holds a few dozen counting waves), of which at most FL_SZ_STREAMS_MAX reach min_bytes
// (FLATE_HIP_INFLATE_SPANS; 0: never).  Appends the indices, ascending.
inline void fl_size_eligible(const uint64_t* in_len, uint32_t n, uint64_t min_bytes, uint32_t n_cu, std::vector<uint32_t>& elig) {
    elig.clear();
    if (!min_bytes) return;
    uint64_t n_long = 0;
    for (uint32_t i = 0; i < n; i++) n_long += in_len[i] >= FL_SZ_LONG_BYTES ? 1u : 0u;
    if (n_long > n_cu) return;
    for (uint32_t i = 0; i < n; i++)
        if (in_len[i] >= min_bytes) elig.push_back(i);
    if (elig.size() > FL_SZ_STREAMS_MAX) elig.clear();
}

// Into how many pieces each eligible stream is cut (1: not at all).  Two pieces per CU over the whole batch, shared
// out by compressed length; a piece has at least FL_SZ_SPAN_BYTES compressed bytes, and the pieces of a call never
// number more than FL_SZ_SPAN_MAX.
inline void fl_size_spacing(const uint64_t* in_len, uint32_t n_elig, uint32_t n_cu, std::vector<uint32_t>& pieces) {
    pieces.assign(n_elig, 1u);
    if (!n_elig || n_elig > FL_SZ_STREAMS_MAX) return;
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_elig; k++) total += in_len[k];
    if (!total) return;
    uint64_t want = 2ull * n_cu;
    if (want > FL_SZ_SPAN_MAX - n_elig) want = FL_SZ_SPAN_MAX - n_elig;  // (every stream keeps one piece whatever its share)
    for (uint32_t k = 0; k < n_elig; k++) {
        // (in_len < 2^32, want <= 1024: the product fits)
        uint64_t p = want * in_len[k] / total;
        const uint64_t most = in_len[k] / FL_SZ_SPAN_BYTES;
        if (p > most) p = most;
        if (p < 1) p = 1;
        pieces[k] = (uint32_t)p;
    }
}

// The scan targets of a stream of in_len bytes cut into p pieces: piece j = 1 .. p - 1 starts at the first block start
// found in [from, limit).  Appends (from_bit, limit_bit) pairs.
inline void fl_size_targets(uint64_t in_len, uint32_t p, std::vector<uint64_t>& from_limit) {
    const uint64_t bits = in_len * 8;
    for (uint32_t j = 1; j < p; j++) {
        from_limit.push_back(bits / p * j);
        from_limit.push_back(j + 1 < p ? bits / p * (j + 1) : bits);
    }
}

// Follow the chain of one stream's spans (ascending start_bit, the first one at the stream's start).  A span is live
// when it starts where the live span before it ended; the chain is closed when every live span has status 0, none of
// its matches reaches further back than the bytes of the live spans before it, and the last live span saw BFINAL.
// Then *size is the sum of the live spans' lengths, *status and *consumed are the last span's.  Anything else
// returns false: the stream is counted whole.
inline bool fl_size_follow_chain(const fl_size_span* sp, const fl_size_rec* rec, uint32_t n, uint64_t* size, int32_t* status,
                                 uint64_t* consumed) {
    if (!n || !sp[0].first) return false;
    uint64_t total = 0;
    uint32_t j = 0;
    for (;;) {
        const fl_size_rec& r = rec[j];
        if (r.status != 0) return false;
        if (r.need_hist > total) return false;
        total += r.out_len;
        if (r.final_seen) {
            *size = total;
            *status = r.status;
            *consumed = r.consumed;
            return true;
        }
        uint32_t k = j + 1;
        while (k < n && sp[k].start_bit < r.end_bit) k++;  // spans that start inside this one are dead
        if (k == n || sp[k].start_bit != r.end_bit) return false;  // a gap: nothing starts where this one ended
        j = k;
    }
}
