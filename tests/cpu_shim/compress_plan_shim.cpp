// CPU build of compress_impl's host decisions (flate_amd/csrc/pass_plan.h): the chunk table, the walk that cuts a batch
// into passes, a pass's block tables, the two-stream rule with its slices, the rectangle rows.
// TEST INFRASTRUCTURE ONLY: lets them be checked without a GPU.  Not linked into libflate_hip.so.
#include "../../flate_amd/csrc/pass_plan.h"

namespace {
fl_pass_cfg cfg_of(uint64_t n_chunks, uint64_t host_pass_chunks, uint64_t max_pass_chunks, int pinned, int ramp, int planned) {
    fl_pass_cfg c;
    c.n_chunks = n_chunks;
    c.host_pass_chunks = host_pass_chunks;
    c.max_pass_chunks = max_pass_chunks;
    c.pinned = pinned != 0;
    c.ramp = ramp != 0;
    c.planned = planned != 0;
    return c;
}
std::vector<fl_chunk> chunks_of(const uint32_t* in_len, uint64_t n) {
    std::vector<fl_chunk> v(n, fl_chunk{});
    for (uint64_t i = 0; i < n; i++) v[i].in_len = in_len[i];
    return v;
}
int put_sched(const std::vector<fl_pass>& v, uint64_t* out, int cap) {
    for (int i = 0; i < (int)v.size() && i < cap; i++) {
        out[3 * i] = v[i].c0;
        out[3 * i + 1] = v[i].nc;
        out[3 * i + 2] = v[i].stream;
    }
    return (int)v.size();
}
struct PlanPass {
    uint32_t nc, nb;
};
}  // namespace

extern "C" {

unsigned shim_sizeof_chunk() { return (unsigned)sizeof(fl_chunk); }

// n + 1 offsets each; `out`: n records.  has_flush: a FlushSpec (its points do not matter here) with this `finish`
int shim_chunk_table(const uint64_t* hin, const uint64_t* hout, uint32_t n, uint64_t in_shift, uint64_t out_shift, int mode,
                     int has_flush, int finish, fl_chunk* out) {
    const FlushSpec fs{nullptr, 0, finish != 0};
    std::vector<fl_chunk> v;
    const bool ok = fl_chunk_table(hin, hout, n, in_shift, out_shift, mode, has_flush ? &fs : nullptr, v);
    for (size_t i = 0; i < v.size(); i++) out[i] = v[i];
    return ok ? 1 : 0;
}

// fl_pass_next from chunk 0 until the batch is covered: up to `cap` (c0, nc, whole-stream) triples, returns the count.
// in_len == NULL: the walk without a chunk table (every chunk on the chunk path)
int shim_pass_walk(const uint32_t* in_len, uint64_t n_chunks, uint64_t host_pass_chunks, uint64_t max_pass_chunks, int pinned,
                   int ramp, int planned, int mode, int has_flush, uint64_t stream_pass_bytes, uint64_t* out, int cap) {
    const fl_pass_cfg c = cfg_of(n_chunks, host_pass_chunks, max_pass_chunks, pinned, ramp, planned);
    std::vector<fl_chunk> chunks;
    if (in_len) chunks = chunks_of(in_len, n_chunks);
    int k = 0;
    for (uint64_t c0 = 0; c0 < n_chunks; k++) {
        const fl_pass_pick pk = fl_pass_next(c, in_len ? chunks.data() : nullptr, c0, (uint64_t)k, mode, has_flush != 0, stream_pass_bytes);
        if (pk.nc == 0) return -1;
        if (k < cap) {
            out[3 * k] = c0;
            out[3 * k + 1] = pk.nc;
            out[3 * k + 2] = pk.stream ? 1 : 0;
        }
        c0 += pk.nc;
    }
    return k;
}

// fl_pass_tables over chunks[0 .. nc) (in place).  Returns nb; *n_blk entries of blk_chunk and *n_sb (start, len, flags)
// triples are what the vectors hold (written up to the caps); st: {tiles, pieces, segs, flush points} of a whole-stream pass
uint32_t shim_pass_tables(fl_chunk* chunks, uint32_t nc, int stream, int mode, int has_flush, const uint64_t* fpos, uint32_t n_fpos,
                          int finish, uint32_t* blk_chunk, uint32_t blk_cap, uint32_t* n_blk, uint32_t* sblocks, uint32_t sb_cap,
                          uint32_t* n_sb, uint32_t* st) {
    const FlushSpec fs{fpos, n_fpos, finish != 0};
    StreamTables tabs;
    std::vector<uint32_t> bc;
    std::vector<fl_sblock> sb;
    const uint32_t nb = fl_pass_tables(chunks, nc, stream != 0, mode, has_flush ? &fs : nullptr, tabs, bc, sb);
    *n_blk = (uint32_t)bc.size();
    *n_sb = (uint32_t)sb.size();
    for (uint32_t i = 0; i < bc.size() && i < blk_cap; i++) blk_chunk[i] = bc[i];
    for (uint32_t i = 0; i < sb.size() && i < sb_cap; i++) {
        sblocks[3 * i] = sb[i].start;
        sblocks[3 * i + 1] = sb[i].len;
        sblocks[3 * i + 2] = sb[i].flags;
    }
    st[0] = (uint32_t)tabs.tiles.size();
    st[1] = (uint32_t)tabs.pieces.size();
    st[2] = (uint32_t)tabs.segs.size();
    st[3] = (uint32_t)tabs.fpts.size();
    return nb;
}

uint64_t shim_batch_blocks(const uint32_t* in_len, uint32_t n, int mode) {
    const std::vector<fl_chunk> chunks = chunks_of(in_len, n);
    return fl_batch_blocks(chunks.data(), n, mode);
}

int shim_two_eligible(const uint32_t* in_len, uint64_t n_chunks, uint64_t host_pass_chunks, uint64_t max_pass_chunks, int pinned, int ramp,
                      int planned, int pinned_passes, uint64_t planned_passes, int mode, int has_flush, int one_stream) {
    const std::vector<fl_chunk> chunks = chunks_of(in_len, n_chunks);
    return fl_two_eligible(cfg_of(n_chunks, host_pass_chunks, max_pass_chunks, pinned, ramp, planned), pinned_passes != 0, (size_t)planned_passes,
                           mode, has_flush != 0, one_stream != 0, chunks.data())
               ? 1
               : 0;
}

// the slices of a plan's passes / of a batch cut here: the schedule as (c0, nc, stream) triples, slice[0..1] = chunks and
// block slots of one slice, *on = two streams.  Returns the number of passes.
int shim_two_from_plan(const uint32_t* nc, const uint32_t* nb, uint32_t n, uint64_t* out, int cap, uint64_t* slice, int* on) {
    std::vector<PlanPass> passes(n);
    for (uint32_t i = 0; i < n; i++) passes[i] = PlanPass{nc[i], nb[i]};
    fl_two_slices s;
    *on = fl_two_from_plan(passes, s) ? 1 : 0;
    slice[0] = s.nc;
    slice[1] = s.nb;
    return put_sched(s.sched, out, cap);
}
int shim_two_from_schedule(uint64_t n_chunks, uint64_t host_pass_chunks, uint64_t max_pass_chunks, int pinned, int ramp, int planned,
                           uint64_t* out, int cap, uint64_t* slice, int* on) {
    fl_two_slices s;
    *on = fl_two_from_schedule(cfg_of(n_chunks, host_pass_chunks, max_pass_chunks, pinned, ramp, planned), s) ? 1 : 0;
    slice[0] = s.nc;
    slice[1] = s.nb;
    return put_sched(s.sched, out, cap);
}

// slot: nc + 1 offsets; out = {urows, pitch, half}
void shim_rect_rows(const uint64_t* slot, uint32_t nc, int rect_knob, uint64_t* out) {
    const fl_rect r = fl_rect_rows(slot, nc, rect_knob);
    out[0] = r.urows;
    out[1] = r.pitch;
    out[2] = r.half;
}

}  // extern "C"
