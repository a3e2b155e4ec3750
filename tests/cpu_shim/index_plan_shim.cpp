// CPU shim over flate_amd/csrc/index_plan.h for tests/test_index_plan_cpu.py: the host decisions of the seek index
// (flate_hip_index_build, flate_hip_decompress_ranges) as plain C functions.
#include "../../flate_amd/csrc/index_plan.h"

extern "C" {

uint64_t shim_idx_const(int i) {
    switch (i) {
        case 0: return FL_IDX_WINDOW;
        case 1: return FL_IDX_SPACING_DEFAULT;
        case 2: return FL_IDX_SLACK;
        case 3: return FL_IDX_SLOT_ALIGN;
        case 4: return FL_IDX_PASS_BYTES;
        case 5: return FL_IDX_HDR_BYTES;
        case 6: return FL_IDX_STREAM_BYTES;
        case 7: return FL_IDX_POINT_BYTES;
        case 8: return FL_IDX_VERSION;
        case 9: return FL_IDX_IN_SPARE;
        default: return 0;
    }
}

int shim_idx_args_ok(int container, int memkind) { return fl_idx_args_ok(container, memkind) ? 1 : 0; }
uint64_t shim_idx_spacing(uint64_t s) { return fl_idx_spacing(s); }
uint64_t shim_idx_max_points(uint64_t size, uint64_t spacing) { return fl_idx_max_points(size, spacing); }
uint32_t shim_idx_window_len(uint64_t out_pos) { return fl_idx_window_len(out_pos); }
uint64_t shim_idx_clip(uint64_t begin, uint64_t len, uint64_t size) { return fl_idx_clip(begin, len, size); }
uint64_t shim_idx_slot_bytes(uint64_t need) { return fl_idx_slot_bytes(need); }

// the point rule over n block positions; which gets the indices, returns their number
uint64_t shim_idx_point_rule(const uint64_t* pos, uint64_t n, uint64_t spacing, uint64_t* which) {
    std::vector<uint64_t> w;
    fl_idx_point_rule(pos, n, spacing, w);
    for (size_t k = 0; k < w.size(); k++) which[k] = w[k];
    return w.size();
}

uint64_t shim_idx_select(const uint64_t* out_pos, uint64_t n, uint64_t begin) {
    std::vector<fl_idx_point> p(n);
    for (uint64_t k = 0; k < n; k++) p[k] = fl_idx_point{0, out_pos[k], 0};
    return fl_idx_select(p.data(), n, begin);
}

// a table of one kind of stream (size, status, its points' positions) repeated; the range of stream `stream`:
// out = point (within the stream) | skip | len | status | decode | in_lo | in_hi; point k's in_bit is in_bit[k] (NULL: k),
// the stream has in_len bytes
void shim_idx_plan_range(uint64_t size, int32_t status, const uint64_t* out_pos, uint64_t n_points, uint32_t n_streams, uint32_t stream,
                         uint64_t begin, uint64_t len, uint64_t cap, uint64_t* out, const uint64_t* in_bit, uint64_t in_len) {
    fl_idx_tab t;
    t.spacing = 1;
    for (uint32_t i = 0; i < n_streams; i++) {
        t.streams.push_back(fl_idx_stream{in_len, size, t.points.size(), n_points, status});
        for (uint64_t k = 0; k < n_points; k++) t.points.push_back(fl_idx_point{in_bit ? in_bit[k] : k, out_pos[k], 0});
    }
    const fl_idx_range r = fl_idx_plan_range(t, stream, begin, len, cap);
    out[0] = r.decode ? r.point - t.streams[stream].point0 : 0;
    out[1] = r.skip;
    out[2] = r.len;
    out[3] = (uint64_t)(int64_t)r.status;
    out[4] = r.decode;
    out[5] = r.in_lo;
    out[6] = r.in_hi;
}

// iv: n lo | hi pairs -> the merged pairs in place, returns their number
uint64_t shim_idx_merge(uint64_t* iv, uint64_t n, uint64_t gap) {
    std::vector<uint64_t> v(iv, iv + 2 * n);
    fl_idx_merge_intervals(v, gap);
    for (size_t k = 0; k < v.size(); k++) iv[k] = v[k];
    return v.size() / 2;
}

// the passes of n ranges; first gets the boundaries (n + 1 entries of room), returns their number less one
uint64_t shim_idx_passes(const uint64_t* slot, uint64_t n, uint64_t budget, uint64_t* first, uint64_t* slot_off, uint64_t* most) {
    std::vector<uint64_t> f, o;
    *most = fl_idx_passes(slot, n, budget, f, o);
    for (size_t k = 0; k < f.size(); k++) first[k] = f[k];
    for (uint64_t j = 0; j < n; j++) slot_off[j] = o[j];
    return f.size() - 1;
}

static void fill_tab(fl_idx_tab& t, uint32_t container, uint64_t spacing, uint32_t ns, const uint64_t* in_len, const uint64_t* size,
                     const int32_t* status, const uint64_t* n_points, const uint64_t* in_bit, const uint64_t* out_pos) {
    t.container = container;
    t.spacing = spacing;
    uint64_t at = 0;
    for (uint32_t i = 0; i < ns; i++) {
        t.streams.push_back(fl_idx_stream{in_len[i], size[i], at, n_points[i], status[i]});
        for (uint64_t k = 0; k < n_points[i]; k++, at++) {
            t.points.push_back(fl_idx_point{in_bit[at], out_pos[at], t.win_bytes});
            t.win_bytes += fl_idx_window_len(out_pos[at]);
        }
    }
}

// blob == NULL: the size; else the blob of the tables, byte b of the windows being (b * 131 + 7) & 255
uint64_t shim_idx_blob(uint32_t container, uint64_t spacing, uint32_t ns, const uint64_t* in_len, const uint64_t* size,
                       const int32_t* status, const uint64_t* n_points, const uint64_t* in_bit, const uint64_t* out_pos, uint8_t* blob) {
    fl_idx_tab t;
    fill_tab(t, container, spacing, ns, in_len, size, status, n_points, in_bit, out_pos);
    if (!blob) return fl_idx_blob_bytes(t);
    const uint64_t at = fl_idx_blob_write(t, blob);
    for (uint64_t b = 0; b < t.win_bytes; b++) blob[at + b] = (uint8_t)(b * 131 + 7);
    return at;
}

// 1: the blob is good, and head = container | spacing | n_streams | n_points | win_bytes | win_at; rows (5 per stream) and
// pts (3 per point) are filled as far as room_streams / room_points allow
int shim_idx_parse(const uint8_t* blob, uint64_t bytes, uint64_t* head, uint64_t* rows, uint64_t room_streams, uint64_t* pts,
                   uint64_t room_points) {
    fl_idx_tab t;
    uint64_t at = 0;
    if (!fl_idx_blob_parse(blob, bytes, t, &at)) return 0;
    head[0] = t.container;
    head[1] = t.spacing;
    head[2] = t.streams.size();
    head[3] = t.points.size();
    head[4] = t.win_bytes;
    head[5] = at;
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
