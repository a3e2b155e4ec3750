// index_plan.h -- host side of the seek index (flate_hip_index_build, flate_hip_decompress_ranges): which block starts
// of a stream are points, which point a byte range starts from, how a range is clipped, how the ranges of a call are cut
// into passes under the scratch budget, where a range's scratch slot lies, and the exported blob: its size, its bytes and
// the validation of one that comes from outside.  Plain C++ (no HIP types): flate_hip.hip uses it, tests/cpu_shim and
// tests/host_cpp compile it for the CPU tests.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "size_plan.h"

#define FL_IDX_WINDOW 32768u              // bytes of history a point carries, at most
#define FL_IDX_SPACING_DEFAULT (1ull << 20)  // spacing 0
#define FL_IDX_SLACK 258u                 // bytes a scratch slot has beyond skip + len: the token that covers the last byte fits whole
#define FL_IDX_IN_SPARE 16u               // input bytes staged behind the block start a range's decode ends at, at most
#define FL_IDX_SLOT_ALIGN 16u             // a scratch slot starts on such a boundary
#define FL_IDX_PASS_BYTES (256ull << 20)  // scratch of one pass of a ranges call (FLATE_HIP_INDEX_PASS_BYTES)
#define FL_IDX_MAGIC 0x58444946u          // "FIDX"
#define FL_IDX_VERSION 1u
#define FL_IDX_HDR_BYTES 48u
#define FL_IDX_STREAM_BYTES 32u
#define FL_IDX_POINT_BYTES 24u
#define FL_IDX_MAX_IN_LEN 0xfffffff0ull   // a stream's compressed length, at most (as every decompress call)

struct fl_idx_stream {
    uint64_t in_len;    // compressed bytes the index was built from
    uint64_t size;      // bytes the first member inflates to (0 unless status is 0)
    uint64_t point0;    // the stream's first point in the table
    uint64_t n_points;  // 0 unless status is 0
    int32_t status;     // of the build's decode
};
struct fl_idx_point {
    uint64_t in_bit;   // the BFINAL bit of a block, counted from the stream's first byte (container header included)
    uint64_t out_pos;  // bytes produced before that block
    uint64_t win_off;  // its window's place among the windows: the min(out_pos, FL_IDX_WINDOW) bytes in front of out_pos
};
struct fl_idx_tab {
    uint32_t container = 0;
    uint64_t spacing = 0;
    std::vector<fl_idx_stream> streams;
    std::vector<fl_idx_point> points;  // stream by stream, ascending
    uint64_t win_bytes = 0;
};

inline uint64_t fl_idx_spacing(uint64_t spacing) { return spacing ? spacing : FL_IDX_SPACING_DEFAULT; }
inline bool fl_idx_args_ok(int container, int memkind) { return container >= 0 && container <= 2 && (memkind == 0 || memkind == 1); }
inline uint32_t fl_idx_window_len(uint64_t out_pos) { return out_pos < FL_IDX_WINDOW ? (uint32_t)out_pos : FL_IDX_WINDOW; }
// points a stream (or a span) of `size` output bytes has, at most: its first block start and one per grid line
inline uint64_t fl_idx_max_points(uint64_t size, uint64_t spacing) { return 1 + size / spacing; }

// The point rule over the block starts of one stream in stream order (pos[k]: bytes produced before block k, pos[0] = 0,
// never descending): block 0 is a point, block k >= 1 is one iff the block in front of it holds a grid line g * spacing
// in (pos[k - 1], pos[k]].  Appends the indices of the points.  The device walker (kernels_index.h) applies the same
// comparison at every block start it passes; this is the statement the tests hold it to.
inline void fl_idx_point_rule(const uint64_t* pos, uint64_t n, uint64_t spacing, std::vector<uint64_t>& which) {
    for (uint64_t k = 0; k < n; k++)
        if (k == 0 || pos[k] / spacing > pos[k - 1] / spacing) which.push_back(k);
}

// The walks of one long stream whose spans the size probe has counted (size_plan.h: ascending spans, their records): one
// walk per live span of the chain, from the span's start to where it ended, with the output bytes of the live spans in
// front of it as its base and room for 1 + out_len / spacing points (the grid lines in (base, base + out_len], and point
// 0 for the first).  false: the chain does not close or does not add up to `size` -- the stream is walked whole.
struct fl_idx_span_walk {
    uint64_t start_bit, stop_bit, base, cap;
    uint32_t first;
};
inline bool fl_idx_span_walks(const fl_size_span* sp, const fl_size_rec* rec, uint32_t n, uint64_t size, uint64_t spacing,
                              std::vector<fl_idx_span_walk>& out) {
    out.clear();
    uint64_t total = 0, used = 0;
    int32_t st = 0;
    if (!fl_size_follow_chain(sp, rec, n, &total, &st, &used) || st != 0 || total != size) return false;
    total = 0;
    for (uint32_t j = 0;;) {
        const fl_size_rec& r = rec[j];
        out.push_back(fl_idx_span_walk{sp[j].start_bit, r.final_seen ? ~0ull : r.end_bit, total, fl_idx_max_points(r.out_len, spacing), sp[j].first});
        total += r.out_len;
        if (r.final_seen) return true;
        while (sp[j].start_bit < r.end_bit) j++;  // (the chain is closed: a span starts where this one ended)
    }
}

// The point a range that begins at `begin` starts from: the last of pts[0 .. n) with out_pos <= begin (n >= 1 and
// pts[0].out_pos == 0: there is one).
inline uint64_t fl_idx_select(const fl_idx_point* pts, uint64_t n, uint64_t begin) {
    uint64_t lo = 0, hi = n;  // pts[lo].out_pos <= begin < pts[hi].out_pos
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (pts[mid].out_pos <= begin) lo = mid; else hi = mid;
    }
    return lo;
}

// bytes of [begin, begin + len) that a stream of `size` bytes has (begin + len may pass 2^64)
inline uint64_t fl_idx_clip(uint64_t begin, uint64_t len, uint64_t size) {
    if (begin >= size) return 0;
    return len < size - begin ? len : size - begin;
}

// The byte intervals [lo, hi) of a host caller's input that a call's decodes can consume, merged where they touch or
// lie at most `gap` bytes apart (a copy has its price): iv holds lo | hi pairs and gets the merged ones, ascending.
inline void fl_idx_merge_intervals(std::vector<uint64_t>& iv, uint64_t gap) {
    const size_t n = iv.size() / 2;
    std::vector<std::pair<uint64_t, uint64_t>> s(n);
    for (size_t k = 0; k < n; k++) s[k] = std::make_pair(iv[2 * k], iv[2 * k + 1]);
    std::sort(s.begin(), s.end());
    std::vector<uint64_t> out;
    for (size_t k = 0; k < n; k++) {
        const uint64_t lo = s[k].first, hi = s[k].second;
        if (hi <= lo) continue;
        if (!out.empty() && lo <= out.back() + (gap < ~0ull - out.back() ? gap : ~0ull - out.back())) {
            if (hi > out.back()) out.back() = hi;
        } else {
            out.push_back(lo);
            out.push_back(hi);
        }
    }
    iv.swap(out);
}

// scratch a range takes that decodes `need` bytes (skip + len) from its point: the bytes, the slack, rounded up to the
// alignment of the next slot
inline uint64_t fl_idx_slot_bytes(uint64_t need) {
    return (need + FL_IDX_SLACK + FL_IDX_SLOT_ALIGN - 1) / FL_IDX_SLOT_ALIGN * FL_IDX_SLOT_ALIGN;
}

// What one range of a call comes to.  decode = 0: the result is known here (status, out_len = 0 bytes: a stream that
// failed in the build, a slot smaller than the clipped length, nothing to deliver).
struct fl_idx_range {
    uint64_t point;  // index into the table's points
    uint64_t skip;   // bytes between the point and the range's first byte
    uint64_t len;    // the clipped length
    uint64_t in_lo, in_hi;  // decode: the bytes of the stream the decode can consume (a host caller's are staged, no others)
    int32_t status;
    uint32_t decode;
};
inline fl_idx_range fl_idx_plan_range(const fl_idx_tab& t, uint32_t stream, uint64_t begin, uint64_t len, uint64_t slot_cap) {
    fl_idx_range r{};
    const fl_idx_stream& s = t.streams[stream];
    if (s.status != 0 || s.n_points == 0) {
        r.status = s.status ? s.status : 1;
        return r;
    }
    r.len = fl_idx_clip(begin, len, s.size);
    if (r.len > slot_cap) {
        r.len = 0;
        r.status = 100;  // FLATE_HIP_ST_OUTPUT_TOO_SMALL
        return r;
    }
    if (r.len == 0) return r;
    const fl_idx_point* pts = t.points.data() + s.point0;
    r.point = s.point0 + fl_idx_select(pts, s.n_points, begin);
    r.skip = begin - t.points[r.point].out_pos;
    // The decode stops at the latest at the first point at or behind the range's end: a block starts there, and with
    // skip + len bytes produced no further block is begun.
    const uint64_t last = fl_idx_select(pts, s.n_points, begin + r.len - 1);
    r.in_lo = t.points[r.point].in_bit >> 3;
    r.in_hi = s.in_len;
    if (last + 1 < s.n_points && (pts[last + 1].in_bit >> 3) + 1 + FL_IDX_IN_SPARE < s.in_len) r.in_hi = (pts[last + 1].in_bit >> 3) + 1 + FL_IDX_IN_SPARE;
    r.decode = 1;
    return r;
}

// The passes of a call: ranges in their order, a pass ends in front of the range that would take its scratch beyond
// `budget`; a range that alone exceeds the budget is a pass of its own.  slot[j]: the scratch of range j (0: it decodes
// nothing).  first gets n_passes + 1 boundaries, slot_off[j] the range's place in its pass's scratch; returns the
// largest pass's scratch.
inline uint64_t fl_idx_passes(const uint64_t* slot, uint64_t n, uint64_t budget, std::vector<uint64_t>& first, std::vector<uint64_t>& slot_off) {
    first.assign(1, 0);
    slot_off.assign(n, 0);
    uint64_t used = 0, most = 0;
    for (uint64_t j = 0; j < n; j++) {
        if (used && slot[j] > budget - (used < budget ? used : budget)) {
            first.push_back(j);
            used = 0;
        }
        slot_off[j] = used;
        used += slot[j];
        if (used > most) most = used;
    }
    if (n) first.push_back(n);
    return most;
}

// ---- the blob: little-endian, no padding, no pointers
//   header   48: magic u32 | version u32 | container u32 | n_streams u32 | spacing u64 | n_points u64 | win_bytes u64 | total u64
//   streams  32 each: in_len u64 | size u64 | status i32 | 0 u32 | n_points u64
//   points   24 each: in_bit u64 | out_pos u64 | win_len u32 | 0 u32
//   windows  win_bytes: the points' windows back to back, in the order of the points
inline void fl_idx_put32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
inline void fl_idx_put64(uint8_t* p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
inline uint32_t fl_idx_get32(const uint8_t* p) { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i); return v; }
inline uint64_t fl_idx_get64(const uint8_t* p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i); return v; }

inline uint64_t fl_idx_blob_bytes(const fl_idx_tab& t) {
    return FL_IDX_HDR_BYTES + (uint64_t)FL_IDX_STREAM_BYTES * t.streams.size() + (uint64_t)FL_IDX_POINT_BYTES * t.points.size() + t.win_bytes;
}
// everything in front of the windows; returns where they go
inline uint64_t fl_idx_blob_write(const fl_idx_tab& t, uint8_t* blob) {
    uint8_t* p = blob;
    fl_idx_put32(p, FL_IDX_MAGIC);
    fl_idx_put32(p + 4, FL_IDX_VERSION);
    fl_idx_put32(p + 8, t.container);
    fl_idx_put32(p + 12, (uint32_t)t.streams.size());
    fl_idx_put64(p + 16, t.spacing);
    fl_idx_put64(p + 24, t.points.size());
    fl_idx_put64(p + 32, t.win_bytes);
    fl_idx_put64(p + 40, fl_idx_blob_bytes(t));
    p += FL_IDX_HDR_BYTES;
    for (const fl_idx_stream& s : t.streams) {
        fl_idx_put64(p, s.in_len);
        fl_idx_put64(p + 8, s.size);
        fl_idx_put32(p + 16, (uint32_t)s.status);
        fl_idx_put32(p + 20, 0);
        fl_idx_put64(p + 24, s.n_points);
        p += FL_IDX_STREAM_BYTES;
    }
    for (const fl_idx_point& q : t.points) {
        fl_idx_put64(p, q.in_bit);
        fl_idx_put64(p + 8, q.out_pos);
        fl_idx_put32(p + 16, fl_idx_window_len(q.out_pos));
        fl_idx_put32(p + 20, 0);
        p += FL_IDX_POINT_BYTES;
    }
    return (uint64_t)(p - blob);
}

// A blob from outside: nothing in it is believed.  true: t holds its tables, *win_at is where its windows start, and
// every invariant the decoder relies on holds -- the counts and the total fit `bytes` exactly, every stream's points are
// its own (a failed stream has none, a good one has point 0 at output byte 0 and at most 1 + size / spacing), in_bit and
// out_pos ascend strictly within a stream, in_bit lies inside the stream, out_pos within its size, and every window has
// min(out_pos, 32768) bytes.
inline bool fl_idx_blob_parse(const uint8_t* blob, uint64_t bytes, fl_idx_tab& t, uint64_t* win_at) {
    t = fl_idx_tab();
    if (!blob || bytes < FL_IDX_HDR_BYTES) return false;
    if (fl_idx_get32(blob) != FL_IDX_MAGIC || fl_idx_get32(blob + 4) != FL_IDX_VERSION) return false;
    const uint32_t container = fl_idx_get32(blob + 8), ns = fl_idx_get32(blob + 12);
    const uint64_t spacing = fl_idx_get64(blob + 16), np = fl_idx_get64(blob + 24), wb = fl_idx_get64(blob + 32);
    if (container > 2 || spacing == 0 || fl_idx_get64(blob + 40) != bytes) return false;
    uint64_t rest = bytes - FL_IDX_HDR_BYTES;
    if (ns > rest / FL_IDX_STREAM_BYTES) return false;
    rest -= (uint64_t)ns * FL_IDX_STREAM_BYTES;
    if (np > rest / FL_IDX_POINT_BYTES) return false;
    rest -= np * FL_IDX_POINT_BYTES;
    if (wb != rest) return false;
    const uint8_t* ps = blob + FL_IDX_HDR_BYTES;
    const uint8_t* pp = ps + (uint64_t)ns * FL_IDX_STREAM_BYTES;
    t.container = container;
    t.spacing = spacing;
    t.streams.resize(ns);
    t.points.resize(np);
    uint64_t at = 0, win = 0;
    for (uint32_t i = 0; i < ns; i++, ps += FL_IDX_STREAM_BYTES) {
        fl_idx_stream& s = t.streams[i];
        s.in_len = fl_idx_get64(ps);
        s.size = fl_idx_get64(ps + 8);
        s.status = (int32_t)fl_idx_get32(ps + 16);
        s.n_points = fl_idx_get64(ps + 24);
        s.point0 = at;
        if (fl_idx_get32(ps + 20) != 0 || s.in_len > FL_IDX_MAX_IN_LEN) return false;
        if (s.status != 0) {
            if (s.n_points != 0 || s.size != 0) return false;
            continue;
        }
        if (s.n_points < 1 || s.n_points > np - at || s.n_points - 1 > s.size / spacing) return false;
        for (uint64_t k = 0; k < s.n_points; k++, pp += FL_IDX_POINT_BYTES) {
            fl_idx_point& q = t.points[at + k];
            q.in_bit = fl_idx_get64(pp);
            q.out_pos = fl_idx_get64(pp + 8);
            q.win_off = win;
            if (fl_idx_get32(pp + 20) != 0 || fl_idx_get32(pp + 16) != fl_idx_window_len(q.out_pos)) return false;
            if (q.in_bit >= s.in_len * 8 || q.out_pos > s.size) return false;
            if (k == 0 ? q.out_pos != 0 : (q.out_pos <= t.points[at + k - 1].out_pos || q.in_bit <= t.points[at + k - 1].in_bit)) return false;
            if (fl_idx_window_len(q.out_pos) > wb - win) return false;
            win += fl_idx_window_len(q.out_pos);
        }
        at += s.n_points;
    }
    if (at != np || win != wb) return false;
    t.win_bytes = wb;
    *win_at = bytes - wb;
    return true;
}
