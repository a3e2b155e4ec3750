// stream_plan.h -- the host decisions of a whole-stream pass (compress_stream_pass in flate_hip.hip, which only carries
// them out): whether the pass may take the windows of k_lz_parse<true> / k_lz_walk<true, true> at all
// (fl_stream_windows_allowed), the window and group tables (fl_stream_windows), the cost estimate that chooses between
// the windows and the sort / match tiles (fl_stream_estimate), the layout of the `wexit` buffer (fl_wexit_offsets), when
// the fix launch is repeated and when the pass is given to the tiles (fl_fix_verdict), which stitch the tiles' parse
// takes and its group tables (fl_stitch_plan), and the workspace bytes of every buffer (fl_stream_ws_*).  Plain C++ (no
// HIP): flate_hip.hip uses it, tests/cpu_shim compiles it for the CPU tests and tests/host_cpp/test_stream_plan.cpp walks
// it under sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "flate_layout.h"
#include "stream_tables.h"

#ifndef FL_STREAM_FIX_MAX
#define FL_STREAM_FIX_MAX 3u  // fix launches of a grouped whole-stream pass before it is handed to the sort / match tiles
#endif

// Round 5: many streams, none of them with flush points, levels 4-7: the demand-driven tokenizer of the chunk path walks
// every stream's windows in order, a workgroup per stream (kernels_parse.h, k_lz_parse<true>) -- no sort, no records for
// every position.  A window costs a workgroup about 0.28 ms, the sort / match pair about 0.061 ms per MiB of all CUs.
// Round 6: levels 8 and 9 the same way on k_lz_links / k_lz_walk<true, true> (kernels_walk.h).
inline bool fl_stream_deep_walk(uint32_t chain) { return chain >= FL_BULK_MIN_CHAIN; }

// (sync-flush points: levels 4-7 only -- k_lz_chain keeps the three positions before a flush point out of the table and
// k_lz_parse<true> ends every match there; the run logic of k_lz_walk counts on runs whose every position is in the table)
// windows_knob: FLATE_HIP_STREAM_WINDOWS (-1 unset, 0 never, 1 whenever possible)
inline bool fl_stream_windows_allowed(bool any_flush, bool deep_walk, int windows_knob, uint32_t nseg) {
    return !(any_flush && deep_walk) && windows_knob != 0 && nseg != 0;
}

// The windows of a pass's streams as chunks (one fl_chunk per 64 KiB window: k_lz_chain / k_lz_links build its chains, the
// tokenizer walks it) and the groups of consecutive windows a workgroup walks.
struct fl_stream_win {
    std::vector<fl_chunk> wch;
    std::vector<fl_swin> sws;
    bool grouped = false;  // some stream is split into groups of windows: a fix launch follows (kernels_parse.h)
    uint32_t G = ~0u;      // windows per group (~0u: a group is a whole stream)
    uint32_t max_win = 0;  // windows of the largest group
    uint64_t bytes = 0;    // uncompressed bytes of the pass
    uint64_t slots = 0;    // workgroups the chip holds at a time
};
// hch: the pass's nc chunks (streams); group_knob: FLATE_HIP_STREAM_GROUP (0: by the number of streams)
inline void fl_stream_windows(const fl_chunk* hch, uint32_t nc, uint32_t group_knob, uint32_t n_cu, bool deep_walk, fl_stream_win& w) {
    w = fl_stream_win();
    uint64_t total_win = 0;
    for (uint32_t i = 0; i < nc; i++) {
        w.bytes += hch[i].in_len;
        total_win += hch[i].n_slides + 1u;
    }
    // Many streams: a workgroup walks a whole stream (no guess, no fix).  Fewer than the chip holds workgroups at a time (one a
    // CU; levels 8-9: two): groups of G windows, as many groups as it holds, so that they all end together and the fix launch
    // -- which parses one window (a sub-pass) per group again -- is one round: G + 1 window times.  (Round 5 took four groups
    // per CU of at least four windows: one 1 MiB stream at level 6 cost 1.9 ms against 1.05 as 32 groups of one window, and
    // 1.34 on the sort / match tiles; one 177 MB stream at level 9 as 675 groups of 8 took 2 x 8 + 2 window times, as 491
    // groups of 11 it takes 11 + 1.  tools/small_stream_round.sh)
    w.slots = deep_walk ? 2ull * n_cu : (uint64_t)n_cu;
    if (nc < w.slots) w.G = (uint32_t)std::max<uint64_t>(1, (total_win + w.slots - 1) / w.slots);
    if (group_knob) w.G = group_knob;
    for (uint32_t i = 0; i < nc; i++) {
        const fl_chunk& c = hch[i];
        const uint32_t nw = c.n_slides + 1u, w0 = (uint32_t)w.wch.size();
        for (uint32_t j = 0; j < nw; j++) {
            fl_chunk wc{};
            wc.in_off = c.in_off + (uint64_t)FL_SEG * j;
            wc.in_len = (uint32_t)std::min<uint64_t>(65536u, (uint64_t)c.in_len - (uint64_t)FL_SEG * j);
            wc.pad_ = 1u;  // (a window: k_lz_chain builds its chains whatever it holds)
            wc.piece0 = FL_SEG * j;  // the window's position in its stream, and the stream's flush points (k_lz_chain)
            wc.flush_off = c.flush_off;
            wc.n_flush = c.n_flush;
            // (+ the bytes behind the window that the lazy calls of its last anchor look at: kernels_parse.h, kernels_walk.h)
            wc.pad_ |= (uint32_t)std::min<uint64_t>(264u, (uint64_t)c.in_len - (uint64_t)FL_SEG * j - wc.in_len) << 8;
            w.wch.push_back(wc);
        }
        uint32_t prev = ~0u;
        for (uint32_t j = 0; j < nw; j += w.G) {
            fl_swin sw{};
            sw.chunk = i;
            sw.win0 = w0 + j;
            sw.nwin = std::min(w.G, nw - j);
            sw.wfirst = j;
            sw.prev = prev;
            prev = (uint32_t)w.sws.size();
            if (j) w.grouped = true;
            w.sws.push_back(sw);
            if (w.G == ~0u) break;
        }
    }
    for (const fl_swin& sw : w.sws) w.max_win = std::max(w.max_win, sw.nwin);
}

// A window costs a workgroup about 0.28 ms (levels 8-9: 1.2, text 1.1, TAR-like 1.6), the fix launch one more per round and
// a host wait; sort / match cost about 0.061 ms per MiB on all CUs (levels 8-9: 0.11 text, 0.20 TAR-like) and 0.8 (1.3) ms
// of kernel latencies whatever the size.  (Measured on MI355X: rounds 5 and 6, tools/small_stream_round.sh.)
constexpr double FL_EST_WIN_MS = 0.28;           // a window on k_lz_parse<true>, levels 4-7
constexpr double FL_EST_WIN_MS_DEEP = 1.5;       // a window on k_lz_walk<true, true>, levels 8-9 (between text and TAR-like)
constexpr double FL_EST_FIX_WAIT_MS = 0.1;       // the host wait of a grouped pass's fix launch
constexpr double FL_EST_TILE_MS_MIB = 0.061;     // sort / match per MiB on all CUs, levels 4-7
constexpr double FL_EST_TILE_MS_MIB_DEEP = 0.11; // ... levels 8-9 (text)
constexpr double FL_EST_TILE_LAT_MS = 0.8;       // kernel latencies of the tiles whatever the size, levels 4-7
constexpr double FL_EST_TILE_LAT_MS_DEEP = 1.3;  // ... levels 8-9
constexpr uint32_t FL_STREAM_ROUND_CAP = 24u;    // rounds of a window's stitch after which a small pass gives it up
constexpr uint64_t FL_STREAM_ROUND_CAP_BYTES = 64ull << 20;  // ... "small": below this many bytes

struct fl_stream_choice {
    bool windows = false;    // the pass takes the windows (else the sort / match tiles)
    uint32_t round_cap = 0;  // rounds of a window's stitch after which the pass is given to the tiles (0: never)
    double est_new = 0, est_old = 0;  // ms: the windows, the tiles
};
// Of a pass that fl_stream_windows_allowed: w its tables, nc its streams, tile_limit FLATE_HIP_MAX_PASS_CHUNKS.  The
// estimate decides only while the knob is unset (< 0).
inline fl_stream_choice fl_stream_estimate(const fl_stream_win& w, uint32_t nc, bool deep_walk, int windows_knob, uint64_t tile_limit) {
    fl_stream_choice c;
    c.windows = true;
    const uint64_t ng = w.sws.size(), slots = w.slots;
    const uint32_t max_win = w.max_win;
    const bool grouped = w.grouped;
    // (a small pass of few streams -- where round 5 took the tiles -- gives a window up after 24 rounds of its stitch: periodic data)
    if (w.bytes < FL_STREAM_ROUND_CAP_BYTES && nc < slots) c.round_cap = FL_STREAM_ROUND_CAP;
    const uint64_t rounds = (ng + slots - 1) / slots;
    const double win_ms = deep_walk ? FL_EST_WIN_MS_DEEP : FL_EST_WIN_MS;
    c.est_new = (double)rounds * max_win * win_ms + (grouped ? (double)rounds * win_ms + FL_EST_FIX_WAIT_MS : 0.0);
    c.est_old = (double)w.bytes / 1048576.0 * (deep_walk ? FL_EST_TILE_MS_MIB_DEEP : FL_EST_TILE_MS_MIB) +
                (deep_walk ? FL_EST_TILE_LAT_MS_DEEP : FL_EST_TILE_LAT_MS);
    if (windows_knob < 0 && c.est_new >= c.est_old) c.windows = false;
    if (w.wch.size() > tile_limit) c.windows = false;  // (the chain links of all windows at once: 128 KiB each)
    return c;
}

// The `wexit` buffer of a pass on the windows, in 32-bit words: per window and sub-pass where the path left it (2 * nw),
// per group its exit (ng) and its entry (ng), and the dirty word (kernels_parse.h, fix launch)
struct fl_wexit_layout {
    uint64_t wexit = 0, gexit = 0, gentry = 0, dirty = 0;  // word offsets
    uint64_t words = 0;                                    // of the whole buffer
};
inline fl_wexit_layout fl_wexit_offsets(uint32_t nw, uint32_t ng) {
    fl_wexit_layout x;
    x.wexit = 0;
    x.gexit = 2 * (uint64_t)nw;
    x.gentry = x.gexit + ng;
    x.dirty = x.gentry + ng;
    x.words = 2 * (uint64_t)nw + 2 * (uint64_t)ng + 4;
    return x;
}

// The groups that were parsed from a guess: again from where the group before them leaves, until nothing moves any more
// (one launch in practice: a parse falls in step within a few bytes; the loop is what makes it exact).  NOT on
// periodic data: in a stream of one repeated byte every anchor is a 258-byte match, a parse from a guessed entry never
// meets the true one, and every launch settles one more group (about ng launches).  After FL_STREAM_FIX_MAX
// launches the pass is given to the sort / match tiles, which cost the same whatever the data.
enum fl_fix { FL_FIX_SETTLED = 0, FL_FIX_AGAIN = 1, FL_FIX_GIVE_UP = 2 };
#define FL_FIX_FIRST 0xffffffffu  // `it` of the read behind the first launch (fix = 0), which no fix launch precedes
// What the dirty word says behind a tokenizer launch: `it` the number of the fix launch it was read behind (0 ..), or
// FL_FIX_FIRST; ng the pass's groups.  AGAIN behind the first launch: the fix launches of a grouped pass follow (a pass
// without groups has none and is settled).
inline fl_fix fl_fix_verdict(uint32_t it, uint32_t flag, uint32_t ng) {
    // (bit 31: some window's stitch did not settle within the round cap -- periodic data -- and its workgroup has stopped)
    if (flag & 0x80000000u) return FL_FIX_GIVE_UP;
    if (it == FL_FIX_FIRST) return FL_FIX_AGAIN;  // (the first launch: nothing but bit 31 is looked at)
    if (!flag) return FL_FIX_SETTLED;
    // (`flag` = the groups that were parsed to their end with a new exit.  Text: none after the first fix launch.  More than
    // an eighth of them: periodic data -- every launch settles one group per stream -- and no reason to try twice more)
    if (it + 1 >= FL_STREAM_FIX_MAX || flag > ng / 8 + 1) return FL_FIX_GIVE_UP;
    return FL_FIX_AGAIN;
}

// The walk from segment to segment behind k_st_parse1: directly for short pieces (k_st_stitch), over groups of
// FL_STITCH_GROUP segments when some piece is long (kernels_stream.h, k_st_stitch_a / _b / _c): then every piece's groups
// in order (an empty piece -- flush called twice -- has none) and where each piece's groups begin.
struct fl_stitch_tables {
    uint32_t max_seg = 0;  // segments of the longest piece
    bool direct = true;
    std::vector<fl_sgroup> groups;  // (grouped stitch only)
    std::vector<uint32_t> group0;   // per piece (grouped stitch only)
};
inline void fl_stitch_plan(const fl_piece* pieces, uint32_t npc, fl_stitch_tables& s) {
    s = fl_stitch_tables();
    for (uint32_t i = 0; i < npc; i++) s.max_seg = std::max(s.max_seg, pieces[i].n_seg);
    s.direct = s.max_seg <= 4 * FL_STITCH_GROUP;
    if (s.direct) return;
    s.group0.resize(npc);
    for (uint32_t i = 0; i < npc; i++) {
        s.group0[i] = (uint32_t)s.groups.size();
        for (uint32_t g = 0; g * FL_STITCH_GROUP < pieces[i].n_seg; g++) s.groups.push_back(fl_sgroup{i, g});
    }
}

// ---- workspace: the bytes of every device buffer of a pass, in the order they are reserved
enum fl_ws_buf {
    FL_WS_TILES = 0, FL_WS_SEGS, FL_WS_PIECES, FL_WS_FPTS, FL_WS_ZONES, FL_WS_NSORTED, FL_WS_CFLAG, FL_WS_S, FL_WS_DESC,
    FL_WS_TOKENS, FL_WS_MARKS, FL_WS_ENTRY, FL_WS_SEGTOK, FL_WS_TOKBASE, FL_WS_BOUND, FL_WS_NTOK,  // every pass
    FL_WS_WCHUNKS, FL_WS_SWINS, FL_WS_LINKS, FL_WS_WEXIT,                                          // the windows
    FL_WS_NC, FL_WS_REC, FL_WS_JMP, FL_WS_EXITMAP,                                                 // the tiles
    FL_WS_SGROUPS, FL_WS_SGROUP0, FL_WS_GMAP, FL_WS_GENTRY,                                        // the grouped stitch
    FL_WS_COUNT
};
struct fl_ws_need {
    fl_ws_buf buf;
    uint64_t bytes;
};
struct fl_ws_list {
    fl_ws_need v[16];
    uint32_t n = 0;
    void add(fl_ws_buf buf, uint64_t bytes) { v[n++] = fl_ws_need{buf, bytes}; }
};

// the sizes of a pass
struct fl_stream_dims {
    uint64_t npos = 0;                      // positions of the per-position arrays (StreamTables::npos)
    uint64_t ntiles = 0, nfpts = 0, nzones = 0;
    uint64_t tiles_per_launch = 0;          // the sort / match tiles run in launches of at most FLATE_HIP_MAX_PASS_CHUNKS
    uint32_t nseg = 0, npc = 0, nb = 0;     // segments, pieces, block slots
    bool deep_walk = false;
};
inline fl_stream_dims fl_stream_dims_of(const StreamTables& t, uint32_t nb, uint64_t tile_limit, bool deep_walk) {
    fl_stream_dims d;
    d.npos = t.npos;
    d.ntiles = t.tiles.size();
    d.nfpts = t.fpts.size();
    d.nzones = t.zones.size();
    d.tiles_per_launch = std::min<uint64_t>(d.ntiles, tile_limit);
    d.nseg = (uint32_t)t.segs.size();
    d.npc = (uint32_t)t.pieces.size();
    d.nb = nb;
    d.deep_walk = deep_walk;
    return d;
}

// ... that every pass needs: its tables, the sort scratch of one launch of tiles, the per-position descriptors, tokens and
// anchor bits, the per-segment and per-piece counts
inline fl_ws_list fl_stream_ws_common(const fl_stream_dims& d) {
    fl_ws_list l;
    l.add(FL_WS_TILES, sizeof(fl_tile) * d.ntiles);
    l.add(FL_WS_SEGS, sizeof(fl_seg) * ((uint64_t)d.nseg + 1));
    l.add(FL_WS_PIECES, sizeof(fl_piece) * (uint64_t)d.npc);
    l.add(FL_WS_FPTS, sizeof(uint32_t) * (d.nfpts + 1));
    l.add(FL_WS_ZONES, sizeof(uint32_t) * (d.nzones + 1));
    l.add(FL_WS_NSORTED, sizeof(uint32_t) * d.tiles_per_launch);
    l.add(FL_WS_CFLAG, sizeof(uint32_t) * d.tiles_per_launch);
    l.add(FL_WS_S, d.tiles_per_launch * FL_CHUNK_STRIDE * sizeof(uint16_t));
    l.add(FL_WS_DESC, d.npos * sizeof(uint32_t));
    l.add(FL_WS_TOKENS, d.npos * sizeof(uint32_t));
    l.add(FL_WS_MARKS, d.npos / 8);
    l.add(FL_WS_ENTRY, sizeof(uint32_t) * ((uint64_t)d.nseg + 1));
    l.add(FL_WS_SEGTOK, sizeof(uint32_t) * ((uint64_t)d.nseg + 1));
    l.add(FL_WS_TOKBASE, sizeof(uint32_t) * ((uint64_t)d.nseg + 1));
    l.add(FL_WS_BOUND, sizeof(uint32_t) * 2 * (uint64_t)d.nb);  // [nb] window positions + [nb] Q1 gaps (k_st_emit)
    l.add(FL_WS_NTOK, sizeof(uint32_t) * (uint64_t)d.npc);
    return l;
}
// (levels 8-9: 512 KiB of links a window -- 16 GiB for a 1 GiB stream; a device that cannot give them: the tiles.  The
// driver asks for them alone and first, because only it can see the device refuse)
inline uint64_t fl_stream_links_bytes(uint32_t nw) { return (uint64_t)nw * FL_CHUNK_STRIDE * 4 * sizeof(uint16_t); }
// ... of a pass on the windows, beside the levels 8-9 links: the two tables, the chain links of levels 4-7 (128 KiB a
// window), a flag word a window, the exits
inline fl_ws_list fl_stream_ws_windows(const fl_stream_dims& d, uint32_t nw, uint32_t ng) {
    fl_ws_list l;
    l.add(FL_WS_WCHUNKS, sizeof(fl_chunk) * (uint64_t)nw);
    l.add(FL_WS_SWINS, sizeof(fl_swin) * (uint64_t)ng);
    if (!d.deep_walk) l.add(FL_WS_S, (uint64_t)nw * FL_CHUNK_STRIDE * sizeof(uint16_t));
    l.add(FL_WS_CFLAG, sizeof(uint32_t) * (uint64_t)nw);
    l.add(FL_WS_WEXIT, sizeof(uint32_t) * fl_wexit_offsets(nw, ng).words);
    return l;
}
// ... what only the sort / match tiles and the stitch over records need (about 14 bytes per input byte): not reserved for a
// pass that takes the windows of k_lz_parse<true>
inline uint64_t fl_stream_rec_bytes(uint64_t npos) { return npos * 2 * sizeof(uint32_t); }  // a record per position
inline fl_ws_list fl_stream_ws_tiles(const fl_stream_dims& d) {
    fl_ws_list l;
    l.add(FL_WS_NC, d.tiles_per_launch * FL_CHUNK_STRIDE * sizeof(uint32_t));
    l.add(FL_WS_REC, fl_stream_rec_bytes(d.npos) + 64);
    l.add(FL_WS_JMP, d.npos * sizeof(uint16_t));
    l.add(FL_WS_EXITMAP, ((uint64_t)d.nseg + 1) * FL_SEG_ENTRIES * sizeof(uint16_t));
    return l;
}
// ... of the grouped stitch: ngr groups in all
inline fl_ws_list fl_stream_ws_stitch(uint32_t ngr, uint32_t npc) {
    fl_ws_list l;
    l.add(FL_WS_SGROUPS, sizeof(fl_sgroup) * ((uint64_t)ngr + 1));
    l.add(FL_WS_SGROUP0, sizeof(uint32_t) * (uint64_t)npc);
    l.add(FL_WS_GMAP, ((uint64_t)ngr + 1) * FL_SEG_ENTRIES * sizeof(uint16_t));
    l.add(FL_WS_GENTRY, sizeof(uint32_t) * ((uint64_t)ngr + 1));
    return l;
}
