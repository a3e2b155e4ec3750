// CPU build of a whole-stream pass's host decisions (flate_amd/csrc/stream_plan.h): the window and group tables, the
// estimate that chooses between windows and tiles, the wexit layout, the fix-launch verdict, the stitch tables, the
// workspace sizes.
// TEST INFRASTRUCTURE ONLY: lets them be checked without a GPU.  Not linked into libflate_hip.so.
#include "../../flate_amd/csrc/stream_plan.h"

namespace {
// the streams of a pass: s[5 * i ..] = {in_off, in_len, n_slides, flush_off, n_flush}
std::vector<fl_chunk> streams_of(const uint64_t* s, uint32_t nc) {
    std::vector<fl_chunk> v(nc, fl_chunk{});
    for (uint32_t i = 0; i < nc; i++) {
        v[i].in_off = s[5 * i];
        v[i].in_len = (uint32_t)s[5 * i + 1];
        v[i].n_slides = (uint32_t)s[5 * i + 2];
        v[i].flush_off = (uint32_t)s[5 * i + 3];
        v[i].n_flush = (uint32_t)s[5 * i + 4];
    }
    return v;
}
int put_list(const fl_ws_list& l, uint64_t* out, int cap) {
    for (int i = 0; i < (int)l.n && i < cap; i++) {
        out[2 * i] = l.v[i].buf;
        out[2 * i + 1] = l.v[i].bytes;
    }
    return (int)l.n;
}
fl_stream_dims dims_of(const uint64_t* d) {  // {npos, ntiles, nfpts, nzones, tile_limit, nseg, npc, nb, deep_walk}
    StreamTables t;
    t.npos = d[0];
    t.tiles.resize(d[1]);
    t.fpts.resize(d[2]);
    t.zones.resize(d[3]);
    t.segs.resize(d[5]);
    t.pieces.resize(d[6]);
    return fl_stream_dims_of(t, (uint32_t)d[7], d[4], d[8] != 0);
}
}  // namespace

extern "C" {

unsigned shim_stream_fix_max() { return FL_STREAM_FIX_MAX; }
unsigned shim_bulk_min_chain() { return FL_BULK_MIN_CHAIN; }
int shim_stream_deep_walk(uint32_t chain) { return fl_stream_deep_walk(chain) ? 1 : 0; }
int shim_stream_windows_allowed(int any_flush, int deep_walk, int windows_knob, uint32_t nseg) {
    return fl_stream_windows_allowed(any_flush != 0, deep_walk != 0, windows_knob, nseg) ? 1 : 0;
}

// wins: per window {in_off, in_len, pad_, piece0, flush_off, n_flush}; groups: per group {chunk, win0, nwin, wfirst, prev};
// meta = {nw, ng, grouped, G, max_win, bytes, slots}.  Both tables are written up to their caps (in entries).
void shim_stream_windows(const uint64_t* streams, uint32_t nc, uint32_t group_knob, uint32_t n_cu, int deep_walk, uint64_t* wins,
                         uint64_t win_cap, uint32_t* groups, uint64_t group_cap, uint64_t* meta) {
    const std::vector<fl_chunk> hch = streams_of(streams, nc);
    fl_stream_win w;
    fl_stream_windows(hch.data(), nc, group_knob, n_cu, deep_walk != 0, w);
    for (uint64_t i = 0; i < w.wch.size() && i < win_cap; i++) {
        const fl_chunk& c = w.wch[i];
        const uint64_t row[6] = {c.in_off, c.in_len, c.pad_, c.piece0, c.flush_off, c.n_flush};
        for (int k = 0; k < 6; k++) wins[6 * i + k] = row[k];
    }
    for (uint64_t i = 0; i < w.sws.size() && i < group_cap; i++) {
        const fl_swin& s = w.sws[i];
        const uint32_t row[5] = {s.chunk, s.win0, s.nwin, s.wfirst, s.prev};
        for (int k = 0; k < 5; k++) groups[5 * i + k] = row[k];
    }
    meta[0] = w.wch.size();
    meta[1] = w.sws.size();
    meta[2] = w.grouped ? 1 : 0;
    meta[3] = w.G;
    meta[4] = w.max_win;
    meta[5] = w.bytes;
    meta[6] = w.slots;
}

// the verdict over the tables of the same pass: returns windows (1) or tiles (0); est = {est_new, est_old}
int shim_stream_estimate(const uint64_t* streams, uint32_t nc, uint32_t group_knob, uint32_t n_cu, int deep_walk, int windows_knob,
                         uint64_t tile_limit, double* est, uint32_t* round_cap) {
    const std::vector<fl_chunk> hch = streams_of(streams, nc);
    fl_stream_win w;
    fl_stream_windows(hch.data(), nc, group_knob, n_cu, deep_walk != 0, w);
    const fl_stream_choice c = fl_stream_estimate(w, nc, deep_walk != 0, windows_knob, tile_limit);
    est[0] = c.est_new;
    est[1] = c.est_old;
    *round_cap = c.round_cap;
    return c.windows ? 1 : 0;
}

void shim_wexit_offsets(uint32_t nw, uint32_t ng, uint64_t* out) {
    const fl_wexit_layout x = fl_wexit_offsets(nw, ng);
    out[0] = x.wexit;
    out[1] = x.gexit;
    out[2] = x.gentry;
    out[3] = x.dirty;
    out[4] = x.words;
}

int shim_fix_verdict(uint32_t it, uint32_t flag, uint32_t ng) { return (int)fl_fix_verdict(it, flag, ng); }

// n_seg: segments of every piece.  meta = {max_seg, direct, groups, group0 entries}; groups as (piece, g) pairs
void shim_stitch_plan(const uint32_t* n_seg, uint32_t npc, uint32_t* groups, uint32_t group_cap, uint32_t* group0, uint32_t* meta) {
    std::vector<fl_piece> pieces(npc, fl_piece{});
    for (uint32_t i = 0; i < npc; i++) pieces[i].n_seg = n_seg[i];
    fl_stitch_tables s;
    fl_stitch_plan(pieces.data(), npc, s);
    for (uint32_t i = 0; i < s.groups.size() && i < group_cap; i++) {
        groups[2 * i] = s.groups[i].piece;
        groups[2 * i + 1] = s.groups[i].g;
    }
    for (uint32_t i = 0; i < s.group0.size(); i++) group0[i] = s.group0[i];
    meta[0] = s.max_seg;
    meta[1] = s.direct ? 1 : 0;
    meta[2] = (uint32_t)s.groups.size();
    meta[3] = (uint32_t)s.group0.size();
}

// shape: 0 common, 1 windows, 2 tiles, 3 grouped stitch (a = ngr, b = npc); a, b: nw, ng of the windows.  (buffer, bytes)
// pairs, returns how many.  dims_out = {tiles_per_launch}
int shim_stream_ws(int shape, const uint64_t* dims, uint32_t a, uint32_t b, uint64_t* out, int cap, uint64_t* dims_out) {
    const fl_stream_dims d = dims_of(dims);
    dims_out[0] = d.tiles_per_launch;
    switch (shape) {
        case 0: return put_list(fl_stream_ws_common(d), out, cap);
        case 1: return put_list(fl_stream_ws_windows(d, a, b), out, cap);
        case 2: return put_list(fl_stream_ws_tiles(d), out, cap);
        default: return put_list(fl_stream_ws_stitch(a, b), out, cap);
    }
}
uint64_t shim_stream_links_bytes(uint32_t nw) { return fl_stream_links_bytes(nw); }
uint64_t shim_stream_rec_bytes(uint64_t npos) { return fl_stream_rec_bytes(npos); }

}  // extern "C"
