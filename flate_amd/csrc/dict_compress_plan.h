// dict_compress_plan.h -- the host decisions of flate_hip_compress_batch_dict (flate_hip.hip, which only carries them
// out): the checks of the call's arguments (fl_dictc_args_ok), the dictionary tail and history length of every stream
// and the too-long verdict (fl_dictc_streams), which streams are staged and which take the ordinary passes
// (fl_dictc_kind), how the batch is cut into passes (fl_dictc_pass_next), where every staged stream lies in the
// staging workspace (fl_dictc_stage), what the pass's chunk table says about a staged stream (fl_dictc_staged_chunks),
// its whole-stream tables (fl_dictc_pass_tables) and the workspace bytes (fl_dictc_ws_bytes).
//
// A stream with a dictionary is compressed as the reference compresses `T ++ R` with a sync flush behind T (T: the last
// min(len, 32768) bytes of the dictionary, R: the record), and what goes out is what follows the flush marker: the
// device sees one stream of D + N bytes whose first D bytes are history only (fl_chunk::hist, stream_tables.h).
// D + N <= 65535, so the reference's window never slides: every such stream is one window.
// Plain C++ (no HIP): tests/cpu_shim compiles it for the CPU tests and tests/host_cpp/test_dict_compress_plan.cpp walks
// it under sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/flate_hip.h"
#include "dict_plan.h"
#include "flate_layout.h"
#include "pass_plan.h"
#include "stream_tables.h"

#define FL_DICTC_MAX_STREAM 65535u  // history + record of one stream: beyond it the reference's window would slide
#ifndef FL_DICTC_PASS_STREAMS
// staged streams per pass: a stream costs its staged bytes, 128 KiB of chain links and about 8 bytes per position of
// per-position arrays (stream_plan.h) -- up to 1 MiB; the chip holds a workgroup per CU at a time (k_lz_parse<true>)
#define FL_DICTC_PASS_STREAMS 2048u
#endif

// What the call may be given: levels 4..9, raw or zlib, and the dictionary arguments of flate_hip_decompress_batch_dict
// (dict_plan.h).  False: FLATE_HIP_E_INVALID_ARG.
inline bool fl_dictc_args_ok(int container, int mode, const uint64_t* dict_off, uint32_t n_dicts, const uint32_t* dict_of,
                             bool have_dict_of, uint32_t n_chunks) {
    if (mode < 4 || mode > 9) return false;
    return fl_dict_args_ok(container, dict_off, n_dicts, dict_of, have_dict_of, n_chunks);
}

// one stream of the call
struct fl_dictc_stream {
    uint32_t dict;     // its dictionary, or FL_DICT_NONE: the stream is compressed as flate_hip_compress_batch does
    uint32_t hist;     // D = min(length of the dictionary, FL_DICT_WINDOW)
    uint64_t t_start;  // dict[t_start, t_start + hist): the dictionary's tail T
};

// The streams of a call (dict_of null: every stream uses dictionary 0).  FLATE_HIP_E_UNSUPPORTED: some stream with a
// dictionary is longer than FL_DICTC_MAX_STREAM with its history; the call does nothing then.
inline int fl_dictc_streams(const uint64_t* hin, uint32_t n_chunks, const std::vector<fl_dict_ent>& tab, const uint32_t* dict_of,
                            std::vector<fl_dictc_stream>& out) {
    out.assign(n_chunks, fl_dictc_stream{FL_DICT_NONE, 0u, 0u});
    for (uint32_t i = 0; i < n_chunks; i++) {
        const uint32_t d = dict_of ? dict_of[i] : 0u;
        if (d == FL_DICT_NONE) continue;
        const fl_dict_ent& e = tab[d];
        out[i].dict = d;
        out[i].hist = e.hist_len;
        out[i].t_start = e.end - e.hist_len;
        if ((uint64_t)e.hist_len + (hin[i + 1] - hin[i]) > FL_DICTC_MAX_STREAM) return FLATE_HIP_E_UNSUPPORTED;
    }
    return FLATE_HIP_OK;
}

// The kinds of pass of such a call: the two of flate_hip_compress_batch (pass_plan.h) for the streams without a
// dictionary, which are not staged, and the staged streams.
enum fl_dictc_kind_t { FL_DICTC_CHUNK = 0, FL_DICTC_STREAM = 1, FL_DICTC_STAGED = 2 };
inline uint32_t fl_dictc_kind(int mode, const fl_dictc_stream& s, uint32_t in_len) {
    if (s.dict != FL_DICT_NONE) return FL_DICTC_STAGED;
    return fl_whole_stream(mode, false, in_len) ? FL_DICTC_STREAM : FL_DICTC_CHUNK;
}

struct fl_dictc_pick {
    uint32_t nc = 0;    // chunks of the pass (never 0 while chunks are left)
    uint32_t kind = 0;  // fl_dictc_kind_t
};
// The pass_index-th pass, which starts at chunk c0: a run of consecutive chunks of one kind.  Chunk passes and
// whole-stream passes end where fl_pass_next ends them; a pass of staged streams holds at most pass_streams of them
// and at most stream_pass_bytes staged bytes (its first stream is always taken).  chunks: the batch's chunk table with
// in_len the record's length.
inline fl_dictc_pick fl_dictc_pass_next(const fl_pass_cfg& cfg, const fl_chunk* chunks, const fl_dictc_stream* ds, uint64_t c0,
                                        uint64_t pass_index, int mode, uint64_t stream_pass_bytes, uint32_t pass_streams) {
    fl_dictc_pick pk;
    pk.kind = fl_dictc_kind(mode, ds[c0], chunks[c0].in_len);
    const uint64_t limit = fl_pass_cap(cfg, c0, pass_index);
    uint64_t bytes = 0, nc = 0;
    for (; c0 + nc < cfg.n_chunks; nc++) {
        const fl_chunk& c = chunks[c0 + nc];
        if (fl_dictc_kind(mode, ds[c0 + nc], c.in_len) != pk.kind) break;
        const uint64_t len = (uint64_t)c.in_len + ds[c0 + nc].hist;
        if (pk.kind == FL_DICTC_CHUNK ? nc >= limit : (nc > 0 && bytes + len > stream_pass_bytes)) break;
        if (pk.kind == FL_DICTC_STAGED && nc >= pass_streams) break;
        bytes += len;
    }
    pk.nc = (uint32_t)nc;
    return pk;
}

// One staged stream of a pass for the staging kernel (kernels_dict.h, k_dict_stage): stage[dst, dst + hist + n) =
// dict[tsrc, tsrc + hist) ++ in[src, src + n)
struct fl_dictc_job {
    uint64_t src, tsrc, dst;
    uint32_t n, hist;
    uint32_t dict;  // index into the call's table of dictionaries (the DICTID of a zlib stream: k_dict_header)
    uint32_t pad_;
};
// a staged stream's bytes in the workspace: whole 16-byte granules, and one more between it and the next
inline uint64_t fl_dictc_stride(uint32_t total) { return (((uint64_t)total + 15u) & ~(uint64_t)15u) + 16u; }
#define FL_DICTC_STAGE_TAIL 256u  // behind the last stream: what the tokenizer's 16-byte loads may read past a stream's end

// Where the nc staged streams of a pass lie (every one at a multiple of 16, none overlapping) and what the staging
// kernel is told.  chunks: the pass's chunks as the caller gave them (in_off, in_len: the record).  Returns the bytes of
// the staging workspace the pass needs.
inline uint64_t fl_dictc_stage(const fl_chunk* chunks, const fl_dictc_stream* ds, uint32_t nc, std::vector<fl_dictc_job>& jobs) {
    jobs.resize(nc);
    uint64_t at = 0;
    for (uint32_t i = 0; i < nc; i++) {
        fl_dictc_job& j = jobs[i];
        j.src = chunks[i].in_off;
        j.tsrc = ds[i].t_start;
        j.dst = at;
        j.n = chunks[i].in_len;
        j.hist = ds[i].hist;
        j.dict = ds[i].dict;
        j.pad_ = 0;
        at += fl_dictc_stride(j.n + j.hist);
    }
    return at + FL_DICTC_STAGE_TAIL;
}

// What the tokenizer and the back end are told about the pass's streams: the input is the staged stream (history and
// record; the pass's kernels read the staging workspace, not the caller's input), and a zlib stream's slot begins four
// bytes later -- the 2-byte header the back end writes there is overwritten by the DICTID, which k_dict_header puts
// behind its own two header bytes at the slot's start.  (A slot of less than four bytes: no room, status 100.)
inline void fl_dictc_staged_chunks(fl_chunk* chunks, const fl_dictc_job* jobs, uint32_t nc, int container) {
    for (uint32_t i = 0; i < nc; i++) {
        fl_chunk& c = chunks[i];
        c.in_off = jobs[i].dst;
        c.in_len = jobs[i].n + jobs[i].hist;
        if (container == FLATE_HIP_ZLIB) {
            c.out_off += 4;
            c.out_cap = c.out_cap >= 4 ? c.out_cap - 4 : 0;
        }
    }
}

// The whole-stream tables of a pass of staged streams (as fl_pass_tables makes them for a pass of streams): a stream
// has one flush point, at its history's end, and its one piece is what follows (an empty dictionary: no flush point at
// all -- the reference's flush of nothing leaves its tokenizer as it was).  Returns the pass's number of blocks.
inline uint32_t fl_dictc_pass_tables(fl_chunk* chunks, const fl_dictc_job* jobs, uint32_t nc, StreamTables& tabs,
                                     std::vector<uint32_t>& blk_chunk) {
    uint32_t nb = 0;
    for (uint32_t i = 0; i < nc; i++) {
        fl_chunk& c = chunks[i];
        c.first_block = nb;
        const uint64_t at = jobs[i].hist;
        const FlushSpec fs{&at, jobs[i].hist ? 1u : 0u, true};
        add_stream_chunk(tabs, c, i, nb, &fs, jobs[i].hist);
        for (uint32_t k = 0; k < c.n_blocks; k++) blk_chunk.push_back(i);
        nb += c.n_blocks;
    }
    return nb;
}

// Device bytes a pass of nc staged streams adds to the workspace of a whole-stream pass (stream_plan.h): the staged
// bytes, the staging kernel's table, and the chunk table of the records for the checksum
inline uint64_t fl_dictc_ws_bytes(uint64_t stage_bytes, uint32_t nc) {
    return stage_bytes + (uint64_t)nc * (sizeof(fl_dictc_job) + sizeof(fl_chunk));
}
