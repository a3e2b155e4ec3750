// CPU shim over flate_amd/csrc/dict_compress_plan.h for tests/test_dict_compress_plan_cpu.py: the host decisions of
// flate_hip_compress_batch_dict as plain C functions.
#include "../../flate_amd/csrc/dict_compress_plan.h"

extern "C" {

uint32_t shim_dictc_const(int i) {
    switch (i) {
        case 0: return FL_DICTC_MAX_STREAM;
        case 1: return FL_DICTC_PASS_STREAMS;
        case 2: return FL_DICTC_STAGE_TAIL;
        case 3: return (uint32_t)sizeof(fl_dictc_job);
        case 4: return (uint32_t)sizeof(fl_chunk);
        default: return 0;
    }
}

int shim_dictc_args_ok(int container, int mode, const uint64_t* dict_off, uint32_t n_dicts, const uint32_t* dict_of,
                       int have_dict_of, uint32_t n_chunks) {
    return fl_dictc_args_ok(container, mode, dict_off, n_dicts, dict_of, have_dict_of != 0, n_chunks) ? 1 : 0;
}

// dict / hist / t_start of every stream; returns the verdict (0, or FLATE_HIP_E_UNSUPPORTED)
int shim_dictc_streams(const uint64_t* hin, uint32_t n_chunks, const uint64_t* dict_off, uint32_t n_dicts, const uint32_t* dict_of,
                       uint32_t* dict, uint32_t* hist, uint64_t* t_start) {
    std::vector<fl_dict_ent> tab;
    fl_dict_table(dict_off, n_dicts, tab);
    std::vector<fl_dictc_stream> ds;
    const int rc = fl_dictc_streams(hin, n_chunks, tab, dict_of, ds);
    for (uint32_t i = 0; i < n_chunks; i++) {
        dict[i] = ds[i].dict;
        hist[i] = ds[i].hist;
        t_start[i] = ds[i].t_start;
    }
    return rc;
}

static void make_batch(const uint64_t* hin, const uint64_t* hout, uint32_t n, const uint32_t* dict, const uint32_t* hist,
                       std::vector<fl_chunk>& chunks, std::vector<fl_dictc_stream>& ds) {
    fl_chunk_table(hin, hout, n, 0, 0, 6, nullptr, chunks);
    ds.resize(n);
    for (uint32_t i = 0; i < n; i++) ds[i] = fl_dictc_stream{dict[i], hist[i], 1000u * i};
}

// the passes of a batch: (nc, kind) pairs; returns how many
uint32_t shim_dictc_passes(const uint64_t* hin, const uint64_t* hout, uint32_t n, const uint32_t* dict, const uint32_t* hist,
                           int mode, uint64_t max_pass_chunks, uint64_t stream_pass_bytes, uint32_t pass_streams, uint32_t* out,
                           uint32_t cap) {
    std::vector<fl_chunk> chunks;
    std::vector<fl_dictc_stream> ds;
    make_batch(hin, hout, n, dict, hist, chunks, ds);
    fl_pass_cfg cfg;
    cfg.n_chunks = n;
    cfg.max_pass_chunks = max_pass_chunks;
    uint32_t k = 0;
    for (uint64_t c0 = 0; c0 < n;) {
        const fl_dictc_pick pk = fl_dictc_pass_next(cfg, chunks.data(), ds.data(), c0, k, mode, stream_pass_bytes, pass_streams);
        if (pk.nc == 0) return ~0u;
        if (k < cap) {
            out[2 * k] = pk.nc;
            out[2 * k + 1] = pk.kind;
        }
        k++;
        c0 += pk.nc;
    }
    return k;
}

// One pass of staged streams, all of the batch: per stream dst / in_off / in_len / out_off / out_cap / n_blocks / n_piece /
// n_flush / first piece's start and end / its tile's tgt0 (11 values); returns the staging bytes; *nb the pass's blocks,
// *ws fl_dictc_ws_bytes
uint64_t shim_dictc_stage(const uint64_t* hin, const uint64_t* hout, uint32_t n, const uint32_t* dict, const uint32_t* hist,
                          int container, uint64_t* rows, uint32_t* nb, uint64_t* ws) {
    std::vector<fl_chunk> chunks;
    std::vector<fl_dictc_stream> ds;
    make_batch(hin, hout, n, dict, hist, chunks, ds);
    std::vector<fl_dictc_job> jobs;
    const uint64_t bytes = fl_dictc_stage(chunks.data(), ds.data(), n, jobs);
    fl_dictc_staged_chunks(chunks.data(), jobs.data(), n, container);
    StreamTables tabs;
    std::vector<uint32_t> blk;
    *nb = fl_dictc_pass_tables(chunks.data(), jobs.data(), n, tabs, blk);
    if (blk.size() != *nb || tabs.tiles.size() != n) return ~0ull;
    for (uint32_t i = 0; i < n; i++) {
        const fl_chunk& c = chunks[i];
        uint64_t* r = rows + 11 * i;
        if (jobs[i].src != hin[i] || jobs[i].tsrc != 1000u * i || jobs[i].dict != dict[i] || c.hist != hist[i]) return ~0ull;
        r[0] = jobs[i].dst;
        r[1] = c.in_off;
        r[2] = c.in_len;
        r[3] = c.out_off;
        r[4] = c.out_cap;
        r[5] = c.n_blocks;
        r[6] = c.n_piece;
        r[7] = c.n_flush;
        r[8] = c.n_piece ? tabs.pieces[c.piece0].start : ~0ull;
        r[9] = c.n_piece ? tabs.pieces[c.piece0].end : ~0ull;
        r[10] = tabs.tiles[i].tgt0;
    }
    *ws = fl_dictc_ws_bytes(bytes, n);
    return bytes;
}
}
