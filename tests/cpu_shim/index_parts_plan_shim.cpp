// CPU shim over flate_amd/csrc/index_parts_plan.h for tests/test_index_parts_plan_cpu.py: the host decisions of the fresh
// seek index (flate_hip_compress_joined_indexed, flate_hip_decompress_ranges on its index) as plain C functions.
#include "../../flate_amd/csrc/index_parts_plan.h"

extern "C" {

uint64_t shim_idxp_const(int i) {
    switch (i) {
        case 0: return FL_IDXP_VERSION;
        case 1: return FL_IDXP_MAX_PARTS;
        default: return 0;
    }
}

// the pieces of a joined stream that are points; which == NULL: their number only
uint64_t shim_idxp_point_pieces(uint64_t n, uint32_t piece, uint64_t spacing, uint64_t* which) {
    std::vector<uint64_t> w;
    fl_idxp_point_pieces(n, piece, spacing, w);
    for (size_t k = 0; which && k < w.size(); k++) which[k] = w[k];
    return w.size();
}

// the points of such a stream from the places of its point pieces: pts gets in_bit | out_pos | win_off rows
void shim_idxp_points(const uint64_t* which, const uint64_t* place, uint64_t n, uint32_t piece, uint64_t* pts) {
    std::vector<fl_idx_point> p;
    fl_idxp_points(which, place, n, piece, p);
    for (size_t k = 0; k < p.size(); k++) {
        pts[3 * k] = p[k].in_bit;
        pts[3 * k + 1] = p[k].out_pos;
        pts[3 * k + 2] = p[k].win_off;
    }
}

static void fill_tab(fl_idx_tab& t, uint32_t container, uint64_t spacing, uint32_t ns, const uint64_t* in_len, const uint64_t* size,
                     const int32_t* status, const uint64_t* n_points, const uint64_t* in_bit, const uint64_t* out_pos) {
    t.container = container;
    t.spacing = spacing;
    uint64_t at = 0;
    for (uint32_t i = 0; i < ns; i++) {
        t.streams.push_back(fl_idx_stream{in_len[i], size[i], at, n_points[i], status[i]});
        for (uint64_t k = 0; k < n_points[i]; k++, at++) t.points.push_back(fl_idx_point{in_bit[at], out_pos[at], 0});
    }
}

// The part table of a call over the given tables.  head = n_parts | n_passes | scratch | n_direct | n_scratch (n_parts =
// ~0: more parts than a call may have, nothing else is written); ranges: part0 | n_parts | len | status rows; parts:
// point | skip | len | dst | in_lo | in_hi | range | direct | slot_off rows, as far as room_parts allows; pass_first
// has room for room_parts + 2 entries.
void shim_idxp_plan_call(uint32_t ns, const uint64_t* in_len, const uint64_t* size, const int32_t* status, const uint64_t* n_points,
                         const uint64_t* in_bit, const uint64_t* out_pos, uint32_t n_ranges, const uint32_t* stream,
                         const uint64_t* begin, const uint64_t* len, const uint64_t* out_off, uint64_t budget, uint64_t* head,
                         uint64_t* ranges, uint64_t* parts, uint64_t room_parts, uint64_t* pass_first) {
    fl_idx_tab t;
    fill_tab(t, 0, 1, ns, in_len, size, status, n_points, in_bit, out_pos);
    fl_idxp_call c;
    if (!fl_idxp_plan_call(t, n_ranges, stream, begin, len, out_off, budget, c)) {
        head[0] = ~0ull;
        return;
    }
    head[0] = c.parts.size();
    head[1] = c.pass_first.size() - 1;
    head[2] = c.scratch;
    head[3] = c.n_direct;
    head[4] = c.n_scratch;
    for (uint32_t j = 0; j < n_ranges; j++) {
        uint64_t* r = ranges + 4 * (size_t)j;
        r[0] = c.ranges[j].part0;
        r[1] = c.ranges[j].n_parts;
        r[2] = c.ranges[j].len;
        r[3] = (uint64_t)(int64_t)c.ranges[j].status;
    }
    for (size_t k = 0; k < c.parts.size() && k < room_parts; k++) {
        const fl_idxp_part& p = c.parts[k];
        uint64_t* r = parts + 9 * k;
        r[0] = p.point;
        r[1] = p.skip;
        r[2] = p.len;
        r[3] = p.dst;
        r[4] = p.in_lo;
        r[5] = p.in_hi;
        r[6] = p.range;
        r[7] = p.direct;
        r[8] = c.slot_off[k];
    }
    for (size_t k = 0; k < c.pass_first.size() && k < room_parts + 2; k++) pass_first[k] = c.pass_first[k];
}

// blob == NULL: the size; else the version-2 blob of the tables
uint64_t shim_idxp_blob(uint32_t container, uint64_t spacing, uint32_t ns, const uint64_t* in_len, const uint64_t* size,
                        const int32_t* status, const uint64_t* n_points, const uint64_t* in_bit, const uint64_t* out_pos, uint8_t* blob) {
    fl_idx_tab t;
    fill_tab(t, container, spacing, ns, in_len, size, status, n_points, in_bit, out_pos);
    if (!blob) return fl_idxp_blob_bytes(t);
    return fl_idxp_blob_write(t, blob);
}

uint32_t shim_idxp_version(const uint8_t* blob, uint64_t bytes) { return fl_idxp_blob_version(blob, bytes); }

// 1: the version-2 blob is good, and head = container | spacing | n_streams | n_points | win_bytes; rows (5 per stream)
// and pts (3 per point) are filled as far as room_streams / room_points allow
int shim_idxp_parse(const uint8_t* blob, uint64_t bytes, uint64_t* head, uint64_t* rows, uint64_t room_streams, uint64_t* pts,
                    uint64_t room_points) {
    fl_idx_tab t;
    if (!fl_idxp_blob_parse(blob, bytes, t)) return 0;
    head[0] = t.container;
    head[1] = t.spacing;
    head[2] = t.streams.size();
    head[3] = t.points.size();
    head[4] = t.win_bytes;
    for (size_t i = 0; i < t.streams.size() && i < room_streams; i++) {
        const fl_idx_stream& s = t.streams[i];
        uint64_t* r = rows + 5 * i;
        r[0] = s.in_len;
        r[1] = s.size;
        r[2] = s.point0;
        r[3] = s.n_points;
        r[4] = (uint64_t)(int64_t)s.status;
    }
    for (size_t k = 0; k < t.points.size() && k < room_points; k++) {
        pts[3 * k] = t.points[k].in_bit;
        pts[3 * k + 1] = t.points[k].out_pos;
        pts[3 * k + 2] = t.points[k].win_off;
    }
    return 1;
}
}
