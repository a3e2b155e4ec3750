// index_parts_plan.h -- host side of the fresh seek index, the one flate_hip_compress_joined_indexed hands out for a
// stream it has just written (index_plan.h: the windowed index flate_hip_index_build makes by decoding): which pieces of
// a joined stream are points and what the points are, how a byte range is cut into parts at the points, the part table
// of a flate_hip_decompress_ranges call on such an index with its passes, and the version-2 blob: its writer and the
// validation of one that comes from outside.  Plain C++ (no HIP types): flate_hip.hip carries it out, tests/cpu_shim and
// tests/host_cpp compile it for the CPU tests.
//
// A fresh point is the start of a piece: the piece was compressed with no history, so a decoder that starts there needs
// no window, and the piece in front of it ends with a sync-flush marker, so the point lies on a byte boundary.
#pragma once
#include <stdint.h>

#include <vector>

#include "index_plan.h"

#define FL_IDXP_VERSION 2u
#define FL_IDXP_MAX_PARTS 0x7fffffffull  // parts of one ranges call: a grid has a workgroup per part

// The pieces of a joined stream of n bytes (pieces of `piece` bytes, join_plan.h) that are points: fl_idx_point_rule
// over the piece starts k * piece with the grid fl_idx_spacing(spacing) -- piece 0, and piece k >= 1 iff a grid line lies
// in ((k - 1) * piece, k * piece].  The rule is fed the starts a stretch at a time (a stream may have 2^31 pieces): a
// stretch begins with the start in front of its own first one, whose verdict (the rule makes every first entry a point)
// is dropped.  Appends the piece numbers, ascending; there are at most 1 + n / spacing of them.
inline void fl_idxp_point_pieces(uint64_t n, uint32_t piece, uint64_t spacing, std::vector<uint64_t>& which) {
    const uint64_t sp = fl_idx_spacing(spacing);
    const uint64_t P = n == 0 ? 1 : n / piece + (n % piece != 0);
    const uint64_t STRETCH = 4096;
    std::vector<uint64_t> pos, got;
    for (uint64_t k0 = 0; k0 < P; k0 += STRETCH) {
        const uint64_t k1 = P - k0 < STRETCH ? P : k0 + STRETCH, lead = k0 ? 1 : 0;
        pos.clear();
        got.clear();
        for (uint64_t k = k0 - lead; k < k1; k++) pos.push_back(k * piece);
        fl_idx_point_rule(pos.data(), pos.size(), sp, got);
        for (uint64_t g : got)
            if (g >= lead) which.push_back(k0 - lead + g);
    }
}

// The points of that stream: place[q] is where piece which[q] begins, in bytes from the stream's first byte (container
// header included) -- k_join_scan's piece_dst less the stream's slot.
inline void fl_idxp_points(const uint64_t* which, const uint64_t* place, uint64_t n, uint32_t piece, std::vector<fl_idx_point>& out) {
    for (uint64_t q = 0; q < n; q++) out.push_back(fl_idx_point{8 * place[q], which[q] * (uint64_t)piece, 0});
}

// ---- a range, cut at the points
// Part of a range: the bytes [max(begin, pos_k), min(begin + L', pos_{k+1} or size)) of the stream, decoded from point k.
struct fl_idxp_part {
    uint64_t point;  // index into the table's points
    uint64_t skip;   // bytes between the point and the part's first byte
    uint64_t len;    // bytes the part delivers (never 0)
    uint64_t dst;    // ... to this offset of the range's slot
    uint64_t in_lo, in_hi;  // the bytes of the stream the decode can consume (a host caller's are staged, no others)
    uint32_t range;
    uint32_t direct;  // skip == 0 and it ends at the next point or at the stream's size: decoded straight into the slot
};
// What one range of a call comes to.  n_parts = 0: the result is known here (status, 0 bytes: a stream that failed, a
// slot smaller than the clipped length, nothing to deliver).
struct fl_idxp_range {
    uint64_t part0, n_parts;  // its parts in the call's table, in stream order
    uint64_t len;             // the clipped length L'
    int32_t status;
};

// scratch a part takes: none when it is direct, else the slot of a range of today (fl_idx_slot_bytes)
inline uint64_t fl_idxp_part_scratch(const fl_idxp_part& p) { return p.direct ? 0 : fl_idx_slot_bytes(p.skip + p.len); }

// Range `range` of a call: [begin, begin + len) of `stream`, clipped as fl_idx_plan_range clips it, into a slot of
// slot_cap bytes.  Returns the number of its parts; parts != nullptr: appends them (part0 is then the table's length
// before).  Per range at most the first and the last part are not direct.
inline uint64_t fl_idxp_cut(const fl_idx_tab& t, uint32_t stream, uint64_t begin, uint64_t len, uint64_t slot_cap, uint32_t range,
                            fl_idxp_range& r, std::vector<fl_idxp_part>* parts) {
    r = fl_idxp_range{};
    r.part0 = parts ? parts->size() : 0;
    const fl_idx_stream& s = t.streams[stream];
    if (s.status != 0 || s.n_points == 0) {
        r.status = s.status ? s.status : 1;
        return 0;
    }
    r.len = fl_idx_clip(begin, len, s.size);
    if (r.len > slot_cap) {
        r.len = 0;
        r.status = 100;  // FLATE_HIP_ST_OUTPUT_TOO_SMALL
        return 0;
    }
    if (r.len == 0) return 0;
    const fl_idx_point* pts = t.points.data() + s.point0;
    const uint64_t end = begin + r.len;  // (<= size)
    const uint64_t first = fl_idx_select(pts, s.n_points, begin), last = fl_idx_select(pts, s.n_points, end - 1);
    r.n_parts = last - first + 1;
    if (!parts) return r.n_parts;
    for (uint64_t k = first; k <= last; k++) {
        const bool more = k + 1 < s.n_points;
        const uint64_t pos = pts[k].out_pos, next = more ? pts[k + 1].out_pos : s.size;
        const uint64_t a = begin > pos ? begin : pos, b = end < next ? end : next;
        fl_idxp_part p{};
        p.point = s.point0 + k;
        p.skip = a - pos;
        p.len = b - a;
        p.dst = a - begin;
        p.range = range;
        p.direct = a == pos && b == next;
        // the decode stops at the latest at the next point: a block starts there (the bit reader looks further ahead)
        p.in_lo = pts[k].in_bit >> 3;
        p.in_hi = s.in_len;
        if (more && (pts[k + 1].in_bit >> 3) + 1 + FL_IDX_IN_SPARE < s.in_len) p.in_hi = (pts[k + 1].in_bit >> 3) + 1 + FL_IDX_IN_SPARE;
        parts->push_back(p);
    }
    return r.n_parts;
}

// The part table of a call and its passes: the ranges in their order, every range's parts in stream order; passes are
// cut over the parts with fl_idx_passes over their scratch (a direct part costs nothing and never opens a pass).
// out_off: the n_ranges + 1 offsets of the slots.  false: more than FL_IDXP_MAX_PARTS parts.
struct fl_idxp_call {
    std::vector<fl_idxp_range> ranges;
    std::vector<fl_idxp_part> parts;
    std::vector<uint64_t> pass_first;  // n_passes + 1 boundaries among the parts
    std::vector<uint64_t> slot_off;    // per part: its place in its pass's scratch
    uint64_t scratch = 0;              // of the largest pass
    uint64_t n_direct = 0, n_scratch = 0;
};
inline bool fl_idxp_plan_call(const fl_idx_tab& t, uint32_t n_ranges, const uint32_t* stream, const uint64_t* begin, const uint64_t* len,
                              const uint64_t* out_off, uint64_t budget, fl_idxp_call& c) {
    c = fl_idxp_call();
    c.ranges.resize(n_ranges);
    uint64_t total = 0;
    for (uint32_t j = 0; j < n_ranges; j++) {
        total += fl_idxp_cut(t, stream[j], begin[j], len[j], out_off[j + 1] - out_off[j], j, c.ranges[j], nullptr);
        if (total > FL_IDXP_MAX_PARTS) return false;
    }
    c.parts.reserve(total);
    for (uint32_t j = 0; j < n_ranges; j++) fl_idxp_cut(t, stream[j], begin[j], len[j], out_off[j + 1] - out_off[j], j, c.ranges[j], &c.parts);
    std::vector<uint64_t> slot(c.parts.size());
    for (size_t p = 0; p < c.parts.size(); p++) {
        slot[p] = fl_idxp_part_scratch(c.parts[p]);
        (c.parts[p].direct ? c.n_direct : c.n_scratch)++;
    }
    c.scratch = fl_idx_passes(slot.data(), slot.size(), budget, c.pass_first, c.slot_off);
    return true;
}

// ---- the version-2 blob: version 1's header and records (index_plan.h) with no windows
//   header   48: magic u32 | 2 u32 | container u32 | n_streams u32 | spacing u64 | n_points u64 | 0 u64 | total u64
//   streams  32 each: in_len u64 | size u64 | status i32 | 0 u32 | n_points u64
//   points   24 each: in_bit u64 | out_pos u64 | 0 u32 | 0 u32
inline uint64_t fl_idxp_blob_bytes(const fl_idx_tab& t) {
    return FL_IDX_HDR_BYTES + (uint64_t)FL_IDX_STREAM_BYTES * t.streams.size() + (uint64_t)FL_IDX_POINT_BYTES * t.points.size();
}
inline uint64_t fl_idxp_blob_write(const fl_idx_tab& t, uint8_t* blob) {
    uint8_t* p = blob;
    fl_idx_put32(p, FL_IDX_MAGIC);
    fl_idx_put32(p + 4, FL_IDXP_VERSION);
    fl_idx_put32(p + 8, t.container);
    fl_idx_put32(p + 12, (uint32_t)t.streams.size());
    fl_idx_put64(p + 16, t.spacing);
    fl_idx_put64(p + 24, t.points.size());
    fl_idx_put64(p + 32, 0);
    fl_idx_put64(p + 40, fl_idxp_blob_bytes(t));
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
        fl_idx_put32(p + 16, 0);
        fl_idx_put32(p + 20, 0);
        p += FL_IDX_POINT_BYTES;
    }
    return (uint64_t)(p - blob);
}

// the version field of a blob (0: too short to have one, or not an index)
inline uint32_t fl_idxp_blob_version(const uint8_t* blob, uint64_t bytes) {
    if (!blob || bytes < 8 || fl_idx_get32(blob) != FL_IDX_MAGIC) return 0;
    return fl_idx_get32(blob + 4);
}

// A version-2 blob from outside: nothing in it is believed.  true: t holds its tables and every invariant the decoder
// relies on holds -- version 1's (fl_idx_blob_parse: the counts and the total fit `bytes` exactly, every stream's points
// are its own, a failed stream has none, a good one has point 0 at output byte 0 and at most 1 + size / spacing, in_bit
// and out_pos ascend strictly within a stream, in_bit lies inside the stream, out_pos within its size), and win_bytes
// and every point's window length are 0.
inline bool fl_idxp_blob_parse(const uint8_t* blob, uint64_t bytes, fl_idx_tab& t) {
    t = fl_idx_tab();
    if (!blob || bytes < FL_IDX_HDR_BYTES) return false;
    if (fl_idx_get32(blob) != FL_IDX_MAGIC || fl_idx_get32(blob + 4) != FL_IDXP_VERSION) return false;
    const uint32_t container = fl_idx_get32(blob + 8), ns = fl_idx_get32(blob + 12);
    const uint64_t spacing = fl_idx_get64(blob + 16), np = fl_idx_get64(blob + 24);
    if (container > 2 || spacing == 0 || fl_idx_get64(blob + 32) != 0 || fl_idx_get64(blob + 40) != bytes) return false;
    uint64_t rest = bytes - FL_IDX_HDR_BYTES;
    if (ns > rest / FL_IDX_STREAM_BYTES) return false;
    rest -= (uint64_t)ns * FL_IDX_STREAM_BYTES;
    if (rest % FL_IDX_POINT_BYTES != 0 || np != rest / FL_IDX_POINT_BYTES) return false;
    const uint8_t* ps = blob + FL_IDX_HDR_BYTES;
    const uint8_t* pp = ps + (uint64_t)ns * FL_IDX_STREAM_BYTES;
    fl_idx_tab u;
    u.container = container;
    u.spacing = spacing;
    u.streams.resize(ns);
    u.points.resize(np);
    uint64_t at = 0;
    for (uint32_t i = 0; i < ns; i++, ps += FL_IDX_STREAM_BYTES) {
        fl_idx_stream& s = u.streams[i];
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
            fl_idx_point& q = u.points[at + k];
            q.in_bit = fl_idx_get64(pp);
            q.out_pos = fl_idx_get64(pp + 8);
            q.win_off = 0;
            if (fl_idx_get32(pp + 16) != 0 || fl_idx_get32(pp + 20) != 0) return false;
            if (q.in_bit >= s.in_len * 8 || q.out_pos > s.size) return false;
            if (k == 0 ? q.out_pos != 0 : (q.out_pos <= u.points[at + k - 1].out_pos || q.in_bit <= u.points[at + k - 1].in_bit)) return false;
        }
        at += s.n_points;
    }
    if (at != np) return false;
    t = std::move(u);
    return true;
}
