// span_plan.h -- host side of the span inflater (kernels_inflate_par.h, "spans"): which streams of a batch are cut and
// where the scan for block starts is aimed, which spans the scan's answers make, whether the records of a stream's spans
// form a closed chain, the work items of k_span_fix, and the fold of their checksum parts against the footer.
// Plain C++ (no HIP types): flate_hip.hip (try_span_inflate) uses it, kernels_inflate_par.h shares the records, and
// tests/cpu_shim compiles it for the CPU tests.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "flate_layout.h"

#define FL_SPAN_MIN_BYTES (128u * 1024u)   // streams shorter than this are not cut (8-32 members of 1 MiB, 130-1000 KB each: 7.0-8.0 -> 5.1-6.2 ms)
#define FL_SPAN_BYTES (64u * 1024u)        // compressed bytes per span, at least
#define FL_SPAN_MAX 1024u                  // spans per call
#ifndef FL_SPAN_STREAMS
#define FL_SPAN_STREAMS 32u
#endif

struct fl_span {
    uint64_t start_bit;  // of its first block header, from the first byte of the stream (first span: unused)
    uint64_t wp;         // run B: offset of its first output byte in the stream's output (run A: 0)
    uint32_t stream;     // chunk index
    uint32_t first;      // 1: starts at the stream's first byte (container header)
    uint32_t prev;       // the span before it in the chain (its tail is this span's history), ~0u: none
    uint32_t live;       // run B: on the chain
};
struct fl_span_res {
    uint64_t end_bit;  // where it stopped: the start of another span, or the bit behind the final block
    uint64_t out_len;
    uint32_t status;      // 0: decoded; anything else: the stream goes the old way
    uint32_t final_seen;  // stopped behind the final block
    uint32_t uses_hist;   // a copy reaches before the span's first byte
    uint32_t n_pieces;    // run A: pieces of the pool taken
};
#define FP_TAIL 32768u
#define FP_NO_SPAN 0xffffffffu
// Run A of a span that is not the first of its stream does not know where its bytes belong: they go to PIECES of a
// pool, taken as the span grows (one atomic per 64 KiB); k_span_fix moves them to their place.
#define FP_PIECE_LOG 16u
#define FP_PIECE (1u << FP_PIECE_LOG)
#define FP_MAX_PIECES 2048u  // per span: 128 MiB of output
// a target of k_span_scan
struct fl_scan_point {
    uint64_t from_bit, limit_bit;  // search [from_bit, limit_bit)
    uint32_t stream, pad;
};
#define FP_FIX_LANE 1024u                 // bytes per lane
#define FP_FIX_ITEM (64u * FP_FIX_LANE)   // ... and item (a wave): a piece of the pool (16 KiB items, 256 bytes a lane: 0.84 -> 1.21 ms)
#define FP_FIX_WAVES 4u                   // items per workgroup: of ONE span, whose history (the true tail before it) they share in LDS
// a work item of k_span_fix (the kinds: kernels_inflate_par.h)
struct fl_fix_item {
    uint64_t dst;    // of the item's first byte in the output buffer
    uint32_t span;   // whose pieces
    uint32_t local;  // offset of the item in the span's output (a multiple of FP_FIX_ITEM)
    uint32_t len;    // <= FP_FIX_ITEM
    uint32_t kind;
    uint32_t prev;   // kind 2: the span before it in the chain
    uint32_t pad;
};
// a stream that came out whole, for k_span_finish
struct fl_span_fin {
    uint64_t total, used;
    uint32_t chunk, pad;
};

// Which streams are cut (ascending indices; none: the batch is decoded a stream at a time), and whether each is cut once.
// Never with min_bytes (FLATE_HIP_INFLATE_SPANS: the minimum stream size in bytes) 0 or the strict header of flags & 1.
struct fl_span_elig {
    std::vector<uint32_t> elig;
    bool twin = false;
};
inline fl_span_elig fl_span_eligible(const fl_chunk* chunks, uint32_t n, uint64_t min_bytes, int flags, uint32_t n_cu, int twin_knob) {
    fl_span_elig e;
    if (!min_bytes || (flags & 1)) return e;
    // Worth it (every span is decoded twice) when the long streams of the batch are too few to fill the chip with
    // a workgroup each: at most FL_SPAN_STREAMS of them (-DFL_SPAN_STREAMS: tuning)
    uint32_t n_long = 0;
    for (uint32_t i = 0; i < n; i++) n_long += chunks[i].in_len >= 32768u ? 1u : 0u;
    // More long streams than that, but fewer than CUs (config #5: 128 members on 256 CUs): every long stream is cut
    // ONCE, where about f = 2 S / (CUs + S) of it lies before the cut, and both runs of the second spans go in one launch
    // with the first spans (TWIN): the CUs the first spans leave free decode the second spans twice in the time the
    // first spans take.  (Cut in two by the rule above, the second run would have half the chip to itself.)  A stream
    // without a place to cut at is one span, decoded in place by run A: as before, but in the same launch.  Config #5,
    // cut at 56 / 62 / 66.6 / 72 / 78 % of the compressed bytes: 11.7 / 7.9 / 6.3 / 6.9 / 7.1 ms -- second spans that
    // are too long cost more than first spans that are: 1.5 % are added to f.
    // twin_knob: FLATE_HIP_SPAN_TWIN -- -1: unset; 0: never; 2..950: where to cut, in thousandths of the stream (tuning)
    e.twin = n_long > FL_SPAN_STREAMS && twin_knob != 0 && (size_t)n_long * 20 <= (size_t)n_cu * 11;  // (40 / 64 / 96 / 160 / 200 one-MiB members: 7.9 / 7.9 / 13.0 / 13.0 / 13.0 ms a workgroup each, 6.1 / 6.1 / 9.1 / 13.3 / 13.4 this way)
    if (n_long > FL_SPAN_STREAMS && !e.twin) return e;
    const uint64_t elig_bytes = e.twin ? std::min<uint64_t>(min_bytes, 32768u) : min_bytes;
    for (uint32_t i = 0; i < n; i++)
        if (chunks[i].in_len >= elig_bytes) e.elig.push_back(i);
    if (e.elig.size() > 256) e.elig.clear();
    return e;
}

// Where spans may start: the targets of k_span_scan (appended), those of stream elig[k] at [pt_first[k], pt_first[k + 1]).
// A span is a workgroup, a workgroup has a CU to itself: as many spans as CUs (a few less: what else runs), or
// a multiple of that for long inputs -- 313 spans on 256 CUs take as long as 499 (measured: 170 MiB of text as
// 249 / 313 / 374 / 499 / 703 spans: 12.3 / 17.5 / 16.2 / 14.3 / 16.3 ms), and every span costs k_span_scan and
// k_span_resolve a step.
// What a span costs goes with the bytes it makes; a stream's share of the spans goes with the room its caller
// gave it (exact for gzip members whose ISIZE was read; 32 bytes per compressed byte at most), a span has at
// least FL_SPAN_BYTES / 4 compressed bytes.
inline uint64_t fl_span_weight(const fl_chunk& c) { return std::max<uint64_t>(c.in_len, std::min<uint64_t>(c.out_cap, 32ull * c.in_len)); }
// sym: one decode per span, in symbols (kernels_inflate_par.h)
inline void fl_span_targets(const fl_chunk* chunks, const std::vector<uint32_t>& elig, bool twin, int twin_knob, bool sym, uint32_t n_cu,
                            std::vector<fl_scan_point>& points, std::vector<uint32_t>& pt_first) {
    pt_first.assign(elig.size() + 1, 0);
    uint64_t elig_w = 0;
    for (uint32_t ci : elig) elig_w += fl_span_weight(chunks[ci]);
    const uint64_t rounds = std::min<uint64_t>(4, std::max<uint64_t>(1, (elig_w + n_cu * 393216ull) / (n_cu * 786432ull)));
    const uint64_t want = std::min<uint64_t>({(uint64_t)FL_SPAN_MAX, rounds * n_cu - std::min<uint32_t>(8u, n_cu / 2), std::max<uint64_t>(2, elig_w / (3 * FL_SPAN_BYTES))});
    for (size_t k = 0; k < elig.size(); k++) {
        const fl_chunk& c = chunks[elig[k]];
        const uint64_t bits = (uint64_t)c.in_len * 8;
        const uint32_t P = twin ? 2u : (uint32_t)std::max<uint64_t>(2, std::min<uint64_t>(want * fl_span_weight(c) / elig_w, c.in_len / (FL_SPAN_BYTES / 4)));
        for (uint32_t j = 1; j < P; j++) {
            fl_scan_point pt;
            // (two runs: f = 2 S / (CUs + S) of the stream before the cut, + 1.5 %; one decode in symbols, 1.25 x the cost of a decode in
            // bytes: f = 1.25 S / (CUs + S / 4))
            const uint64_t auto_f = sym ? std::min<uint64_t>(900, std::max<uint64_t>(500, 1250ull * elig.size() / (n_cu + elig.size() / 4) + 10))
                                        : std::min<uint64_t>(900, std::max<uint64_t>(500, 2000ull * elig.size() / (n_cu + elig.size()) + 15));
            pt.from_bit = twin ? bits / 1000 * (twin_knob > 1 ? (uint64_t)std::min(950, twin_knob) : auto_f) : bits / P * j;
            pt.limit_bit = j + 1 < P ? bits / P * (j + 1) : bits;
            pt.stream = elig[k];
            pt.pad = 0;
            points.push_back(pt);
        }
        pt_first[k + 1] = (uint32_t)points.size();
    }
}

// The positions a stream is cut at: every distinct position found[j0 .. j1) names, ascending (the targets are), below
// limit_bit.  ~0: the scan found nothing for that target.
inline std::vector<uint64_t> fl_cut_positions(const uint64_t* found, uint32_t j0, uint32_t j1, uint64_t limit_bit) {
    std::vector<uint64_t> pos;
    uint64_t last = 0;
    for (uint32_t j = j0; j < j1; j++) {
        if (found[j] == ~0ull || found[j] <= last || found[j] >= limit_bit) continue;
        last = found[j];
        pos.push_back(found[j]);
    }
    return pos;
}

// The spans (appended): for every eligible stream its start, then every position it is cut at; those of stream elig[k] at
// [sp_first[k], sp_first[k + 1]).  cand holds the cut positions alone, those of chunk i at [cand_off[i], cand_off[i + 1]).
inline void fl_span_build(uint32_t n_chunks, const std::vector<uint32_t>& elig, const std::vector<uint32_t>& pt_first, const uint64_t* found,
                          std::vector<fl_span>& spans, std::vector<uint64_t>& cand, std::vector<uint32_t>& cand_off, std::vector<uint32_t>& sp_first) {
    cand_off.assign(n_chunks + 1, 0);
    sp_first.assign(elig.size() + 1, 0);
    size_t k = 0;
    for (uint32_t i = 0; i < n_chunks; i++) {
        cand_off[i] = (uint32_t)cand.size();
        if (k == elig.size() || elig[k] != i) continue;
        fl_span s = {/*start_bit*/ 0, /*wp*/ 0, /*stream*/ i, /*first*/ 1, /*prev*/ FP_NO_SPAN, /*live*/ 0};
        spans.push_back(s);
        s.first = 0;
        for (uint64_t p : fl_cut_positions(found, pt_first[k], pt_first[k + 1], ~0ull)) {
            s.start_bit = p;
            spans.push_back(s);
            cand.push_back(p);
        }
        sp_first[++k] = (uint32_t)spans.size();
    }
    cand_off[n_chunks] = (uint32_t)cand.size();
}

// Pieces of the pool run A writes to: what the streams can hold (at most 32 bytes for every compressed one: beyond
// that a stream goes the old way), two pieces of slack per span; twice that where run B writes to the pool as well.
// (A pool the device cannot give -- callers who reserve the worst case for gigabytes of input: the old way.  The
// pool is a second copy of the decoded output: never more than FL_SPAN_POOL_MAX, so that an allocator that shares the
// device -- PyTorch's -- is not starved.)
#define FL_SPAN_POOL_MAX (16ull << 30)
inline uint64_t fl_span_pool_pieces(const fl_chunk* chunks, const std::vector<uint32_t>& elig, uint32_t nsp, bool both) {
    uint64_t bytes = 0;
    for (uint32_t ci : elig) bytes += std::min<uint64_t>(chunks[ci].out_cap, 32ull * chunks[ci].in_len);
    return ((bytes >> FP_PIECE_LOG) + 2ull * nsp + 1) * (both ? 2 : 1);
}

// The chain of one stream, whose spans are spans[a .. b) (ascending start_bit, the first one at the stream's start) with
// run A's records r1: from the first span to the span that starts where it stopped, and so on to the span that stopped
// behind the final block.  A span on the chain gets live = 1, wp = the bytes before it and prev = the span before it
// (the numbers are those of the whole array).  A chain that does not close -- a status, a gap, more bytes than out_cap,
// no final block -- clears live on the whole stream: it is decoded the old way.
struct fl_span_chain {
    bool ok = false;
    std::vector<uint32_t> chain;
    uint64_t total = 0, end_bit = 0;  // bytes of the chain's spans (failed: as far as the walk came); where the final block ended
    uint32_t last = 0;                // the span the walk looked at last
};
inline fl_span_chain fl_span_follow_chain(fl_span* spans, const fl_span_res* r1, uint32_t a, uint32_t b, uint64_t out_cap, bool both) {
    fl_span_chain pl;
    uint32_t cur = a;
    uint64_t acc = 0;
    bool ok = a < b;
    for (uint32_t guard = 0; ok && guard <= b - a; guard++) {
        const fl_span_res& r = r1[cur];
        pl.last = cur;
        if (r.status != 0) { ok = false; break; }
        // (run B of a twin launch does not know where its span starts: a distance that reaches before the start of
        // the OUTPUT -- possible in the first 32 KiB only -- is the old path's to find)
        if (both && !spans[cur].first && r.uses_hist && acc < FP_TAIL) { ok = false; break; }
        spans[cur].live = 1;
        spans[cur].wp = acc;
        spans[cur].prev = pl.chain.empty() ? FP_NO_SPAN : pl.chain.back();
        pl.chain.push_back(cur);
        acc += r.out_len;
        if (acc > out_cap || acc < r.out_len) { ok = false; break; }  // (a sum that wraps: no device record says so; refused like any other overrun)
        if (r.final_seen) { pl.end_bit = r.end_bit; break; }
        // the span that starts where this one stopped
        uint32_t lo = a + 1, hi = b;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (spans[mid].start_bit < r.end_bit) lo = mid + 1; else hi = mid;
        }
        if (lo >= b || spans[lo].start_bit != r.end_bit || lo <= cur) { ok = false; break; }
        cur = lo;
    }
    if (ok && (pl.chain.empty() || !r1[pl.chain.back()].final_seen)) ok = false;
    if (!ok)
        for (uint32_t j = a; j < b; j++) spans[j].live = 0;
    pl.ok = ok;
    pl.total = acc;
    return pl;
}

// What follows run A: the closed chains one after another (chain_all; stream k's at [chain_off[k], chain_off[k + 1]),
// every span's place in its chain and the longest chain for the k_span_rs_* steps) and the work items of k_span_fix,
// stream k's at [item_first[k], item_first[k + 1]): FP_FIX_ITEM bytes of a span each, at dst = out_off + wp + local.
struct fl_span_fix_plan {
    std::vector<uint32_t> chain_all, chain_off, chain_pos;
    uint32_t longest = 0;
    bool uses_hist = false;
    std::vector<fl_fix_item> items;
    std::vector<uint32_t> item_first;
};
inline fl_span_fix_plan fl_span_fix_items(const fl_chunk* chunks, const std::vector<uint32_t>& elig, const fl_span* spans, const fl_span_res* r1,
                                          const std::vector<fl_span_chain>& plans, uint32_t nsp, bool both) {
    fl_span_fix_plan fp;
    fp.chain_off.push_back(0);
    for (const fl_span_chain& pl : plans) {
        if (pl.ok) {
            fp.chain_all.insert(fp.chain_all.end(), pl.chain.begin(), pl.chain.end());
            for (uint32_t j = 0; j < pl.chain.size(); j++) fp.chain_pos.push_back(j);
            fp.longest = std::max<uint32_t>(fp.longest, (uint32_t)pl.chain.size());
        }
        fp.chain_off.push_back((uint32_t)fp.chain_all.size());
    }
    // (streams without a single copy that reaches before its span -- huffman-only, store-only ones -- need neither
    // run B nor the true tails)
    for (uint32_t si : fp.chain_all) fp.uses_hist = fp.uses_hist || r1[si].uses_hist != 0;
    fp.item_first.assign(elig.size() + 1, 0);
    for (size_t k = 0; k < elig.size(); k++) {
        if (plans[k].ok) {
            for (uint32_t si : plans[k].chain) {
                const uint64_t n = r1[si].out_len;
                for (uint64_t o = 0; o < n; o += FP_FIX_ITEM) {
                    fl_fix_item it;
                    it.dst = chunks[elig[k]].out_off + spans[si].wp + o;
                    it.span = si;
                    it.local = (uint32_t)o;
                    it.len = (uint32_t)std::min<uint64_t>(FP_FIX_ITEM, n - o);
                    it.kind = spans[si].first ? 0u : fp.uses_hist ? (both ? 3u : 2u) : 1u;
                    it.prev = spans[si].prev;
                    it.pad = both ? nsp : 0u;
                    fp.items.push_back(it);
                }
                // (a workgroup of k_span_fix takes FP_FIX_WAVES items of ONE span: empty ones fill the last)
                while (fp.items.size() % FP_FIX_WAVES) {
                    fl_fix_item it = fp.items.back();
                    it.local = 0;
                    it.len = 0;
                    fp.items.push_back(it);
                }
            }
        }
        fp.item_first[k + 1] = (uint32_t)fp.items.size();
    }
    return fp;
}

// The container's footer: its length, and where in the stream the footer of a closed chain lies (the byte behind the
// final block; ~0: the stream ends before it does)
inline uint32_t fl_span_footer_len(int container) { return container == 1 ? 8u : container == 2 ? 4u : 0u; }
inline uint64_t fl_span_footer_at(const fl_span_chain& pl, uint32_t flen, uint64_t in_len) {
    const uint64_t fb = (pl.end_bit + 7) >> 3;
    return pl.ok && fb + flen <= in_len ? fb : ~0ull;
}

// A closed chain after k_span_fix: run B as run A (where there was a run B: uses_hist; the first span's run A was
// final), the checksum of the stream folded from its items' parts (part[2 q]: the CRC-32 of item q, or its Adler-32
// from a = b = 0; part[2 q + 1]: its length) in stream order, and the footer (foot: its bytes; gzip CRC, ISIZE little
// endian; zlib Adler-32 big endian).  pow_item: x^(8 FP_FIX_ITEM) of xpow8 (fl_crc_consts).  A footer that the
// stream is too short for is the old way's to name.  used: the stream's bytes, footer included.
struct fl_span_verdict {
    bool ok = true;
    uint64_t used = 0;
    uint32_t crc = 0;
    uint32_t bad_b = ~0u;  // the place in the chain of the span whose run B differs (~0: none)
};
inline fl_span_verdict fl_span_verify(const fl_span_chain& pl, const fl_span* spans, const fl_span_res* r1, const fl_span_res* r2, bool uses_hist,
                                      const uint32_t* part, uint32_t n_parts, int container, const uint32_t* xpow8, uint32_t pow_item,
                                      const uint8_t* foot, uint64_t in_len) {
    fl_span_verdict v;
    for (size_t j = 0; j < pl.chain.size() && v.ok && uses_hist; j++) {
        const uint32_t si = pl.chain[j];
        if (spans[si].first) continue;  // (run A was final)
        const fl_span_res &a = r1[si], &b = r2[si];
        if (b.status != 0 || b.out_len != a.out_len || b.end_bit != a.end_bit) {
            v.ok = false;
            v.bad_b = (uint32_t)j;
        }
    }
    uint64_t adA = 0, adB = 0;  // Adler-32 with a = b = 0 start
    for (uint32_t q = 0; q < n_parts && v.ok; q++) {
        const uint32_t pc = part[2 * (size_t)q], plen = part[2 * (size_t)q + 1];
        if (container == 1) {
            v.crc = fl_crc_mulmod(v.crc, plen == FP_FIX_ITEM ? pow_item : fl_crc_xpow8n(xpow8, plen)) ^ pc;
        } else if (container == 2) {
            adB = (adB + adA * plen + (pc >> 16)) % 65521u;
            adA = (adA + (pc & 0xffff)) % 65521u;
        }
    }
    const uint32_t flen = fl_span_footer_len(container);
    const uint64_t fb = (pl.end_bit + 7) >> 3;
    v.used = fb + flen;
    if (v.ok && fb + flen > in_len) v.ok = false;  // truncated: the old way names it
    if (v.ok && flen) {
        const uint8_t* f = foot;
        if (container == 1) {
            const uint32_t fcrc = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
            const uint32_t fsz = (uint32_t)f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) | ((uint32_t)f[7] << 24);
            v.ok = fcrc == v.crc && fsz == (uint32_t)pl.total;
        } else {
            const uint32_t a = (uint32_t)((1 + adA) % 65521u);
            const uint32_t b = (uint32_t)((pl.total % 65521u + adB) % 65521u);
            const uint32_t fad = ((uint32_t)f[0] << 24) | ((uint32_t)f[1] << 16) | ((uint32_t)f[2] << 8) | (uint32_t)f[3];
            v.ok = fad == ((b << 16) | a);
        }
    }
    return v;
}
