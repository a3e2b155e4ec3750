// CPU build of the host side of a resumable huffman-only / store-only feed (flate_amd/csrc/deflater_plan.h).
// TEST INFRASTRUCTURE ONLY: lets the block schedule the deflater builds on the host be checked against the one-shot
// block lists and the oracle, and a feed's check, routing, layout and settle rule be checked without a GPU.  Not linked
// into libflate_hip.so.
#include "../../flate_amd/csrc/deflater_plan.h"

// a stream's mirror as the tests pass it: bl, hdr_done, finished, pend_len, pend_pos
static fl_dfl_mirror mirror_in(const uint64_t* v) {
    fl_dfl_mirror m;
    m.bl = (uint32_t)v[0];
    m.hdr_done = (uint8_t)v[1];
    m.finished = (uint8_t)v[2];
    m.pend_len = v[3];
    m.pend_pos = v[4];
    return m;
}
static void mirror_out(const fl_dfl_mirror& m, uint64_t* v) {
    v[0] = m.bl;
    v[1] = m.hdr_done;
    v[2] = m.finished;
    v[3] = m.pend_len;
    v[4] = m.pend_pos;
}

extern "C" {

// blocks of one feed: writes up to `cap` (start, len, flags) triples, returns the count; *keep = bytes left buffered
int shim_dfl_blocks(uint32_t bl, uint32_t n, int op, uint32_t* out, int cap, uint32_t* keep) {
    std::vector<fl_sblock> v;
    *keep = fl_dfl_blocks(bl, n, op, v);
    for (int i = 0; i < (int)v.size() && i < cap; i++) {
        out[3 * i] = v[i].start;
        out[3 * i + 1] = v[i].len;
        out[3 * i + 2] = v[i].flags;
    }
    return (int)v.size();
}

int shim_dfl_checksum_units(uint32_t bl, uint32_t n, uint32_t* out, int cap) {
    std::vector<fl_sblock> v;
    fl_dfl_checksum_units(bl, n, v);
    for (int i = 0; i < (int)v.size() && i < cap; i++) {
        out[2 * i] = v[i].start;
        out[2 * i + 1] = v[i].len;
    }
    return (int)v.size();
}

uint64_t shim_dfl_out_bound(uint32_t bl, uint32_t n) { return fl_dfl_out_bound(bl, n); }

uint64_t shim_dfl_max_piece() { return FL_DFL_MAX_PIECE; }

int shim_dfl_feed_ok(const uint64_t* hin, const uint64_t* hout, const uint8_t* hop, uint32_t n, int have_in) {
    return fl_dfl_feed_ok(hin, hout, hop, n, have_in != 0) ? 1 : 0;
}

// mirror: in and out; out: from, give, status; returns the kind
int shim_dfl_route(uint64_t* mirror, uint64_t piece, int op, uint64_t slot, uint64_t* out) {
    fl_dfl_mirror m = mirror_in(mirror);
    const fl_dfl_route r = fl_dfl_route_stream(m, piece, op, slot);
    mirror_out(m, mirror);
    out[0] = r.from;
    out[1] = r.give;
    out[2] = (uint64_t)r.status;
    return r.kind;
}

uint32_t shim_dfl_stage_slices(uint64_t max_units) { return fl_dfl_stage_slices(max_units); }

// The layout of the streams act[0..nj) of a deflater of n streams whose mirrors are 5 values each.  jobs: nj x 9 -- src_off,
// stream, bl, n, keep, ck_first, ck_n, hdr, finish; chunks: nj x 8 -- in_off, in_len, out_off, out_cap, first_block,
// n_blocks, unfinished, and 1 where every other byte of the entry is 0; blocks and units: up to cap x 4 -- start, len, flags,
// job; totals: win_n, out_n, max_units, slices, blocks, units.  Returns 0 where a table's length is not what it has to be.
int shim_dfl_lay_out(const uint64_t* mirrors, uint32_t n, const uint32_t* act, uint32_t nj, const uint64_t* hin, const uint8_t* hop,
                     int dev, uint64_t* jobs, uint64_t* chunks, uint64_t* blocks, uint64_t* units, uint64_t cap, uint64_t* totals) {
    std::vector<fl_dfl_mirror> mir(n);
    for (uint32_t i = 0; i < n; i++) mir[i] = mirror_in(mirrors + 5 * i);
    fl_dfl_layout lay;
    lay.jobs.resize(7);  // (what an earlier feed left must go)
    lay.win_n = 99;
    fl_dfl_lay_out(mir.data(), std::vector<uint32_t>(act, act + nj), hin, hop, dev != 0, lay);
    if (lay.jobs.size() != nj || lay.chunks.size() != nj || lay.block_job.size() != lay.blocks.size() ||
        lay.unit_job.size() != lay.units.size())
        return 0;
    for (uint32_t j = 0; j < nj; j++) {
        const fl_dfl_job& jb = lay.jobs[j];
        const uint64_t row[9] = {jb.src_off, jb.stream, jb.bl, jb.n, jb.keep, jb.ck_first, jb.ck_n, jb.hdr, jb.finish};
        memcpy(jobs + 9 * j, row, sizeof row);
        fl_chunk c = lay.chunks[j];
        const uint64_t crow[7] = {c.in_off, c.in_len, c.out_off, c.out_cap, c.first_block, c.n_blocks, c.unfinished};
        memcpy(chunks + 8 * j, crow, sizeof crow);
        c.in_off = c.out_off = c.out_cap = 0;
        c.in_len = c.first_block = c.n_blocks = c.unfinished = 0;
        const fl_chunk zero{};
        chunks[8 * j + 7] = memcmp(&c, &zero, sizeof c) == 0;
    }
    for (uint64_t k = 0; k < lay.blocks.size() && k < cap; k++) {
        const uint64_t row[4] = {lay.blocks[k].start, lay.blocks[k].len, lay.blocks[k].flags, lay.block_job[k]};
        memcpy(blocks + 4 * k, row, sizeof row);
    }
    for (uint64_t k = 0; k < lay.units.size() && k < cap; k++) {
        const uint64_t row[4] = {lay.units[k].start, lay.units[k].len, lay.units[k].flags, lay.unit_job[k]};
        memcpy(units + 4 * k, row, sizeof row);
    }
    const uint64_t t[6] = {lay.win_n, lay.out_n, lay.max_units, lay.slices, lay.blocks.size(), lay.units.size()};
    memcpy(totals, t, sizeof t);
    return 1;
}

// mirror: in and out; the job by its n, keep and finish; out: give, pend, consumed, status; returns ok
int shim_dfl_settle(uint64_t* mirror, uint32_t n, uint32_t keep, uint32_t finish, uint64_t out_cap, uint64_t produced, uint64_t slot,
                    uint64_t* out) {
    fl_dfl_mirror m = mirror_in(mirror);
    fl_dfl_job jb{};
    jb.n = n;
    jb.keep = keep;
    jb.finish = finish;
    fl_chunk ck{};
    ck.out_cap = out_cap;
    const fl_dfl_settled s = fl_dfl_settle(m, jb, ck, produced, slot);
    mirror_out(m, mirror);
    out[0] = s.give;
    out[1] = s.pend;
    out[2] = s.consumed;
    out[3] = (uint64_t)s.status;
    return s.ok ? 1 : 0;
}
}
