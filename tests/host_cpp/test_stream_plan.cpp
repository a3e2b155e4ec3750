// A whole-stream pass's host-side decisions (flate_amd/csrc/stream_plan.h) over random passes, hostile ones among them:
// zero-length streams, a single stream at the length limit, thousands of tiny streams, groups of one window, flush points
// on top of each other.  The tables come from add_stream_chunk, so flush points and zones are what a call would make.
// Built with -fsanitize=address,undefined by tests/test_host_cpp.py; needs no GPU.  It checks invariants -- the groups
// partition every stream's windows in order, no window looks beyond its stream, the stitch groups cover every segment
// once, the regions of the wexit buffer do not overlap, the fix loop ends -- not what the rules decide
// (tests/test_stream_plan_cpu.py does).
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../flate_amd/csrc/stream_plan.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}
static uint64_t below(uint64_t n) { return rnd() % n; }

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            printf("line %d: %s (set %d)\n", __LINE__, #c, set_no); \
            return 1;                                               \
        }                                                           \
    } while (0)

static uint64_t windows_seen = 0, groups_seen = 0, stitch_groups_seen = 0;

// every rule over one pass
static int walk_pass(int set_no, const std::vector<fl_chunk>& hch, const StreamTables& t, uint32_t nb, uint32_t group_knob, uint32_t n_cu,
                     bool deep_walk, int windows_knob, uint64_t tile_limit) {
    const uint32_t nc = (uint32_t)hch.size();
    // ---- windows and groups
    fl_stream_win w;
    fl_stream_windows(hch.data(), nc, group_knob, n_cu, deep_walk, w);
    const uint32_t nw = (uint32_t)w.wch.size(), ng = (uint32_t)w.sws.size();
    CHECK(w.slots == (deep_walk ? 2ull : 1ull) * n_cu && w.G >= 1);
    uint64_t bytes = 0;
    uint32_t w0 = 0, g = 0;
    bool grouped = false;
    for (uint32_t i = 0; i < nc; i++) {
        const fl_chunk& c = hch[i];
        const uint32_t n = c.n_slides + 1u;
        CHECK((uint64_t)w0 + n <= nw);
        for (uint32_t j = 0; j < n; j++) {
            const fl_chunk& wc = w.wch[w0 + j];
            const uint32_t look = wc.pad_ >> 8;
            CHECK((wc.pad_ & 0xffu) == 1u && look <= 264u && wc.in_len <= 65536u);
            CHECK(wc.in_off == c.in_off + (uint64_t)FL_SEG * j && wc.piece0 == FL_SEG * j);
            CHECK(wc.in_off + wc.in_len + look <= c.in_off + c.in_len);
            CHECK(j + 1 == n ? wc.in_off + wc.in_len == c.in_off + c.in_len : wc.in_len == 65536u);
            CHECK(wc.flush_off == c.flush_off && wc.n_flush == c.n_flush);
        }
        // the stream's groups: in order, back to back, each linked to the one before
        uint32_t at = 0, prev = ~0u;
        for (; g < ng && w.sws[g].chunk == i; g++) {
            const fl_swin& sw = w.sws[g];
            CHECK(sw.win0 == w0 + at && sw.wfirst == at && sw.prev == prev);
            CHECK(sw.nwin >= 1 && sw.nwin <= w.G && sw.nwin <= w.max_win && (uint64_t)sw.win0 + sw.nwin <= nw);
            CHECK(at + sw.nwin == n || sw.nwin == w.G);  // only a stream's last group is short
            if (at) grouped = true;
            at += sw.nwin;
            prev = g;
        }
        CHECK(at == n);
        w0 += n;
        bytes += c.in_len;
    }
    CHECK(w0 == nw && g == ng && bytes == w.bytes && grouped == w.grouped);
    CHECK(nc == 0 || w.G == ~0u || group_knob == w.G || nc < w.slots);
    windows_seen += nw;
    groups_seen += ng;
    // ---- the verdict
    const uint32_t nseg = (uint32_t)t.segs.size();
    const bool allowed = fl_stream_windows_allowed(t.any_flush, deep_walk, windows_knob, nseg);
    CHECK(!(t.any_flush && deep_walk && allowed) && !(windows_knob == 0 && allowed) && !(nseg == 0 && allowed));
    const fl_stream_choice ch = fl_stream_estimate(w, nc, deep_walk, windows_knob, tile_limit);
    CHECK(std::isfinite(ch.est_new) && std::isfinite(ch.est_old) && ch.est_new >= 0 && ch.est_old > 0);
    CHECK(ch.round_cap == 0 || (ch.round_cap == 24 && w.bytes < (64ull << 20) && nc < w.slots));
    CHECK(!(nw > tile_limit && ch.windows));
    CHECK(!(windows_knob > 0 && nw <= tile_limit && !ch.windows));
    // ---- the wexit buffer: four regions, one behind the other, inside the buffer
    const fl_wexit_layout x = fl_wexit_offsets(nw, ng);
    CHECK(x.wexit == 0 && x.wexit + 2ull * nw <= x.gexit && x.gexit + ng <= x.gentry && x.gentry + ng <= x.dirty && x.dirty + 1 <= x.words);
    // ---- the fix loop as the driver runs it, on whatever the device might answer: it ends
    {
        uint32_t launches = 0;
        fl_fix v = fl_fix_verdict(FL_FIX_FIRST, below(4) ? 0u : (uint32_t)rnd(), ng);
        CHECK(v == FL_FIX_AGAIN || v == FL_FIX_GIVE_UP);
        for (uint32_t it = 0; w.grouped && v == FL_FIX_AGAIN; it++) {
            launches++;
            const uint32_t flag = below(3) ? (uint32_t)below(ng / 8 + 3) : below(2) ? 0u : (uint32_t)rnd();
            v = fl_fix_verdict(it, flag, ng);
            CHECK(v == FL_FIX_SETTLED || v == FL_FIX_AGAIN || v == FL_FIX_GIVE_UP);
            CHECK(flag != 0 || v == FL_FIX_SETTLED);
            CHECK(!(flag & 0x80000000u) || v == FL_FIX_GIVE_UP);
        }
        CHECK(launches <= FL_STREAM_FIX_MAX);
    }
    // ---- the stitch: every segment of every piece in one group, once
    fl_stitch_tables s;
    fl_stitch_plan(t.pieces.data(), (uint32_t)t.pieces.size(), s);
    CHECK(s.direct == (s.max_seg <= 4 * FL_STITCH_GROUP));
    if (s.direct) {
        CHECK(s.groups.empty() && s.group0.empty());
        for (const fl_piece& pc : t.pieces) CHECK(pc.n_seg <= 4 * FL_STITCH_GROUP);
    } else {
        CHECK(s.group0.size() == t.pieces.size());
        uint64_t covered = 0, k = 0;
        for (uint32_t i = 0; i < t.pieces.size(); i++) {
            CHECK(s.group0[i] == k);
            for (uint32_t gi = 0; gi * FL_STITCH_GROUP < t.pieces[i].n_seg; gi++, k++) {
                CHECK(k < s.groups.size() && s.groups[k].piece == i && s.groups[k].g == gi);
                covered += std::min(FL_STITCH_GROUP, t.pieces[i].n_seg - gi * FL_STITCH_GROUP);
            }
        }
        CHECK(k == s.groups.size() && covered == nseg);
        stitch_groups_seen += k;
    }
    // ---- the workspace lists: known buffers, each once, and the sizes that must agree with each other
    const fl_stream_dims d = fl_stream_dims_of(t, nb, tile_limit, deep_walk);
    CHECK(d.tiles_per_launch <= tile_limit && d.tiles_per_launch <= t.tiles.size() && d.nseg == nseg);
    const fl_ws_list lists[4] = {fl_stream_ws_common(d), fl_stream_ws_windows(d, nw, ng), fl_stream_ws_tiles(d),
                                 fl_stream_ws_stitch((uint32_t)s.groups.size(), (uint32_t)t.pieces.size())};
    for (const fl_ws_list& l : lists) {
        CHECK(l.n >= 1 && l.n <= 16);
        uint64_t seen = 0;
        for (uint32_t i = 0; i < l.n; i++) {
            CHECK((uint32_t)l.v[i].buf < (uint32_t)FL_WS_COUNT && !(seen >> l.v[i].buf & 1));
            seen |= 1ull << l.v[i].buf;
            if (l.v[i].buf == FL_WS_WEXIT) CHECK(l.v[i].bytes == 4 * x.words);
            if (l.v[i].buf == FL_WS_REC) CHECK(l.v[i].bytes >= fl_stream_rec_bytes(t.npos));
            if (l.v[i].buf == FL_WS_DESC || l.v[i].buf == FL_WS_TOKENS) CHECK(l.v[i].bytes == 4 * t.npos);
        }
    }
    CHECK(fl_stream_links_bytes(nw) == (uint64_t)nw * 524288u);
    return 0;
}

int main() {
    const uint32_t cus[] = {1, 2, 8, 256, 304};
    uint64_t passes = 0;
    for (int set_no = 0; set_no < 1500; set_no++) {
        const bool hostile = set_no % 3 == 0;
        // ---- the streams of the pass: a flush call has one (possibly empty), a batch has streams above 65535 bytes
        const bool flush = below(4) == 0;
        const uint32_t nc = flush ? 1u : set_no % 100 == 7 ? 3000u + (uint32_t)below(3000) : 1 + (uint32_t)below(below(4) ? 6 : 400);
        std::vector<fl_chunk> hch(nc, fl_chunk{});
        StreamTables t;
        uint32_t nb = 0;
        uint64_t in_off = below(1u << 20);
        std::vector<uint64_t> fpos;
        for (uint32_t i = 0; i < nc; i++) {
            uint64_t len;
            switch (below(8)) {
                case 0: len = flush && hostile ? 0 : 65536; break;
                case 1: len = 65536 + below(3) * 32768 + below(3) - 1; break;
                case 2: len = 131072 + 262 + below(5); break;
                case 3: len = nc > 1000 ? below(200000) : below(20) ? below(5000000) : 8400000 + below(3000000); break;  // (above 8 MiB: the grouped stitch)
                default: len = nc > 1000 ? 1 + below(70000) : below(400000); break;
            }
            if (!flush && nc <= 1000 && len <= 65535) len += 65536;
            fl_chunk& c = hch[i];
            c.in_off = in_off;
            c.in_len = (uint32_t)len;
            in_off += len + below(64);
            if (flush) {
                uint64_t at = 0;
                for (uint64_t k = below(6); k > 0; k--) {
                    at += hostile && below(3) == 0 ? 0 : below(len - at + 1);  // (flush called twice: an empty piece)
                    fpos.push_back(at);
                }
            }
            const FlushSpec fs{fpos.data(), (uint32_t)fpos.size(), below(2) != 0};
            c.first_block = nb;
            add_stream_chunk(t, c, i, nb, flush ? &fs : nullptr);
            nb += c.n_blocks;
        }
        const uint32_t group_knob = below(3) ? 0u : 1 + (uint32_t)below(hostile ? 2 : 20);   // (G of 1 among them)
        const uint32_t n_cu = cus[below(5)];
        const uint64_t tile_limit = below(3) ? 32768 : 1 + below(64);
        if (walk_pass(set_no, hch, t, nb, group_knob, n_cu, below(2) != 0, (int)below(3) - 1, tile_limit)) return 1;
        passes++;
    }
    // ---- a single stream at the length limit of levels 4..9 (fl_chunk_table), through the tables; and one at 4 GiB - 16,
    // where stream positions end, through the window rules alone (no tile table reaches that far)
    {
        const int set_no = -1;
        for (const uint32_t n_cu : {1u, 256u}) {
            std::vector<fl_chunk> hch(1, fl_chunk{});
            StreamTables t;
            hch[0].in_len = 0xfff00000u;
            add_stream_chunk(t, hch[0], 0, 0, nullptr);
            CHECK(hch[0].n_slides + 1u == 0xfff00000u / FL_SEG);
            if (walk_pass(set_no, hch, t, hch[0].n_blocks, 0, n_cu, n_cu == 1, -1, 32768)) return 1;
            if (walk_pass(set_no, hch, t, hch[0].n_blocks, 1, n_cu, false, 1, ~0ull)) return 1;
            passes += 2;
        }
        fl_chunk c{};
        c.in_off = 12345;
        c.in_len = 0xfffffff0u;
        c.n_slides = (c.in_len - 65536u) / FL_SEG + 1;
        fl_stream_win w;
        fl_stream_windows(&c, 1, 0, 304, true, w);
        CHECK(w.wch.size() == c.n_slides + 1u && w.bytes == c.in_len && w.G == (w.wch.size() + 607) / 608);
        const fl_chunk& last = w.wch.back();
        CHECK(last.in_off + last.in_len == c.in_off + c.in_len && last.piece0 == FL_SEG * c.n_slides && (last.pad_ >> 8) == 0);
        uint64_t sum = 0;
        for (const fl_swin& sw : w.sws) {
            CHECK(sw.win0 == sum && sw.wfirst == sum);
            sum += sw.nwin;
        }
        CHECK(sum == w.wch.size());
    }
    printf("ok: %llu passes, %llu windows in %llu groups, %llu stitch groups\n", (unsigned long long)passes,
           (unsigned long long)windows_seen, (unsigned long long)groups_seen, (unsigned long long)stitch_groups_seen);
    return passes > 1500 && stitch_groups_seen > 0 ? 0 : 2;
}
